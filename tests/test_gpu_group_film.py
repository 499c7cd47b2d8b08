"""Group films on the MI355X (include/ykgpu.h "group films"): a film over the k
entries of a device group is, byte for byte, the single-context film of the same params.  Every
comparison is on bytes, with no tolerance: against the reference-generated goldens, against the
numpy yardsticks (film_ref, film_adaptive_ref, film_denoise_ref, film_features_ref) and against a
single-context film.  One device, groups [0] * k: repeated entries run the very path a node runs
(one context, streams and buffers per entry; the exchange's copies and event waits between them).
The shapes are the smallest at which each mechanism can go wrong: entries without rows, bands
shorter than the halo, a halo as tall as the tile, row and column subsets, per-pixel counts.
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
from uecraytracing_amd.records import (PRECISION_FP32, RNG_XOR128, SEED_RANDOM_DEVICE, DenoiseParams, FeatureParams,
                                       GroupDenoiseStats, make_params)

pytestmark = pytest.mark.gpu

CAM = refscenes.reference_camera()
MAN = golden_data.manifest()
YK_ERR_INVALID, YK_ERR_UNSUPPORTED = 1, 4
REF4_6 = dict(width=32, height=18, spp=6, max_depth=50, seed0=404)
MIXED_16 = dict(width=32, height=18, spp=16, max_depth=50, seed0=404)


@pytest.fixture(scope="module")
def ren():
    r = yk.Renderer(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def groups():
    """Group [0] * k per k, made on first use and kept for the module."""
    made = {}

    def get(k):
        if k not in made:
            made[k] = yk.Group([0] * k)
        return made[k]

    yield get
    for g in made.values():
        g.close()


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def golden(name):
    return next(c for c in MAN["cases"] if c["name"] == name)


def state(film):
    sums, sumsq, _ = film.read()
    return sums, sumsq, film.counts()


def put(film, sums, sumsq, counts):
    film.write_counts(sums, sumsq, np.broadcast_to(np.asarray(counts, np.uint32), film._shape))


def same_state(a, b, what):
    for x, y, name in zip(state(a), state(b), ("sums", "second moments", "counts")):
        assert same(x, y), f"{name} {what}"
    assert a.done == b.done and a.count_range() == b.count_range(), what


def mixed_prefixes(p=None):
    p = p or make_params(**MIXED_16)
    return film_ref.prefixes(film_ref.colours(refscenes.mixed12(), CAM, p))


# ---- 1. golden parity -----------------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("mode,suffix", [(dict(), ""), (dict(precision=PRECISION_FP32), "_f32"),
                                         (dict(rng=RNG_XOR128), "_x128")], ids=["fp64", "fp32", "xor128"])
def test_golden_parity_in_chunks(ren, groups, k, mode, suffix):
    entry = golden("ref4_32x18x6_d50_s404" + suffix)
    p = make_params(**REF4_6, **mode)
    g = groups(k)
    g.set_scene(refscenes.ref4(), CAM)
    ren.set_scene(refscenes.ref4(), CAM)
    with g.film(p) as gf, ren.film(p) as sf:
        assert bytes(gf.params) == bytes(sf.params)
        done = 0
        for n in (1, 2, 3):
            assert gf.accumulate(n) == done + n == sf.accumulate(n)
            done += n
            same_state(gf, sf, f"after {done}")
            assert same(gf.resolve(), sf.resolve())
            tot, per = g.stats(-1), [g.stats(e) for e in range(k)]
            assert tot["samples"] == 32 * 18 * n == sum(s["samples"] for s in per)
            assert [s["samples"] for s in per] == [len(range(e, 18, k)) * 32 * n for e in range(k)]
            assert tot["launches"] == sum(s["launches"] for s in per) >= k
        sums, _, d = gf.read()
        assert d == 6 and same(sums, golden_data.sums(entry))
        assert same(gf.resolve(), golden_data.rgb(entry))
        with pytest.raises(yk.YkError, match="YK_ERR_INVALID.*target"):
            gf.accumulate(1)
        with pytest.raises(yk.YkError, match="YK_ERR_INVALID"):
            gf.accumulate(0)


# ---- 2. tiles -------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,tile", [(5, dict(rows=(10, 3, 1))), (3, dict(cols=(3, 21, 1))), (3, dict(rows=(1, 7, 2))),
                                    (3, dict(rows=(1, 7, 2), cols=(2, 9, 3)))],
                         ids=["3-rows-5-entries", "columns", "row-stride-2", "rows-and-columns"])
def test_tiles(ren, groups, k, tile):
    p = make_params(**REF4_6, **tile)
    g = groups(k)
    g.set_scene(refscenes.ref4(), CAM)
    ren.set_scene(refscenes.ref4(), CAM)
    whole = golden_data.sums(golden("ref4_32x18x6_d50_s404"))
    with g.film(p) as gf, ren.film(p) as sf:
        for n in (2, 4):
            gf.accumulate(n)
            sf.accumulate(n)
            same_state(gf, sf, f"{tile} after {n}")
        sums, _, _ = gf.read()
        ys, xs = film_ref.tile_rows(p), film_ref.tile_cols(p)
        assert same(sums, np.ascontiguousarray(whole[ys][:, xs]))
        assert same(gf.resolve(), sf.resolve())
        e2, st = gf.error(0.0)
        e2s, sts = sf.error(0.0)
        assert same(e2, e2s) and st == sts
        if k == 5:  # the entries without rows hold nothing and did nothing
            assert g.stats(3)["samples"] == 0 and g.stats(4)["samples"] == 0


def test_banded_rows_are_not_dealt(groups):
    g = groups(2)
    g.set_scene(refscenes.ref4(), CAM)
    with pytest.raises(yk.YkError, match="YK_ERR_UNSUPPORTED.*row_band_log2"):
        g.film(make_params(**REF4_6, rows=(0, 8, 2, 1)))
    g1 = groups(1)  # one entry deals nothing: the film is the context's own
    g1.set_scene(refscenes.ref4(), CAM)
    with g1.film(make_params(**REF4_6, rows=(0, 8, 2, 1))) as gf:
        gf.accumulate(2)
        assert gf.done == 2


# ---- 3. keyed seeds -------------------------------------------------------------------------------

def test_random_device_key_is_drawn_once_for_every_entry(ren, groups):
    g = groups(3)
    g.set_scene(refscenes.ref4(), CAM)
    ren.set_scene(refscenes.ref4(), CAM)
    with g.film(make_params(**REF4_6, seed_mode=SEED_RANDOM_DEVICE)) as gf:
        key = gf.params.seed_key
        assert key != 0
        gf.accumulate(2)
        gf.accumulate(4)
        assert g.stats(-1)["seed_key"] == key and all(g.stats(e)["seed_key"] == key for e in range(3))
        with ren.film(make_params(**REF4_6, seed_mode=SEED_RANDOM_DEVICE, seed_key=key)) as sf:
            sf.accumulate(6)
            assert bytes(sf.params) == bytes(gf.params)
            same_state(gf, sf, "keyed")


# ---- 4. adaptive passes ---------------------------------------------------------------------------

def check_against_sim(film, sim, what):
    sums, sumsq, counts = state(film)
    assert same(counts, sim.counts), f"counts {what}"
    assert same(sums, sim.sums()) and same(sumsq, sim.sumsq()), f"sums {what}"
    assert film.done == int(sim.counts.min()), what
    assert film.count_range() == (int(sim.counts.min()), int(sim.counts.max())), what
    assert same(film.resolve(), sim.image()), f"image {what}"


def adaptive_pass(gf, sf, sim, thr2, n, what):
    got = gf.accumulate_adaptive(thr2, n).as_dict()
    one = sf.accumulate_adaptive(thr2, n).as_dict()
    want = sim.step(thr2, n)
    print(what, "threshold2", thr2, "reference", want, "single", one, "group", got)
    for key in ("pixels_selected", "samples_added", "min_count", "max_count"):
        assert got[key] == one[key] == want[key], (what, key)
    # groups and launches are sums over the entries: no fewer than the single film's
    assert got["groups"] >= one["groups"] and got["launches"] >= one["launches"]
    check_against_sim(gf, sim, what)
    same_state(gf, sf, what)
    return want


def test_adaptive_passes(ren, groups):
    p = make_params(**MIXED_16)
    g = groups(3)
    g.set_scene(refscenes.mixed12(), CAM)
    ren.set_scene(refscenes.mixed12(), CAM)
    sim = far.Sim(film_ref.colours(refscenes.mixed12(), CAM, p))
    with g.film(p) as gf, ren.film(p) as sf:
        gf.accumulate(4)
        sf.accumulate(4)
        assert sim.step(-1.0, 4)["pixels_selected"] == 32 * 18
        check_against_sim(gf, sim, "after the uniform chunk")
        thr2 = sim.threshold2(0.5)
        for i in range(3):
            want = adaptive_pass(gf, sf, sim, thr2, 4, f"pass {i}")
            assert 0 < want["pixels_selected"] < 32 * 18  # (the precondition: some but not all)
            tot = g.stats(-1)
            assert tot["samples"] == want["samples_added"] == sum(g.stats(e)["samples"] for e in range(3))
        assert sim.counts.min() != sim.counts.max()
        with pytest.raises(yk.YkError, match="YK_ERR_INVALID.*different sample counts"):
            gf.accumulate(1)
        e2, st = gf.error(thr2)
        e2s, sts = sf.error(thr2)
        assert same(e2, e2s) and same(e2, sim.e2()) and st == sts
        # an empty pass: nothing selected, nothing launched
        done = adaptive_pass(gf, sf, sim, float("inf"), 4, "nothing over +inf")
        assert done["pixels_selected"] == 0 and g.stats(-1)["launches"] == 0
        adaptive_pass(gf, sf, sim, -1.0, 16, "to the target")
        assert gf.count_range() == (16, 16) and same(gf.read()[0], ren.render_sums(p))


# ---- 5. entries that are each uniform, at different counts ------------------------------------------

def test_mixed_uniform_entries(ren, groups):
    p = make_params(**REF4_6)
    g = groups(2)
    g.set_scene(refscenes.ref4(), CAM)
    ren.set_scene(refscenes.ref4(), CAM)
    S, Q = film_ref.prefixes(film_ref.colours(refscenes.ref4(), CAM, p))
    counts = np.zeros((18, 32), np.uint32)
    counts[0::2], counts[1::2] = 4, 6  # the rows of entry 0 and of entry 1
    with g.film(p) as gf, ren.film(p) as sf:
        for f in (gf, sf):
            put(f, far.at_counts(S, counts), far.at_counts(Q, counts), counts)
        lib = gf._lib
        assert lib.ykgpu_group_film_accumulate(gf._f, 1) == YK_ERR_INVALID
        assert b"different sample counts" in lib.ykgpu_last_error()
        assert gf.done == 4 == sf.done and gf.count_range() == (4, 6)
        same_state(gf, sf, "mixed")
        assert same(gf.resolve(), sf.resolve()) and same(gf.resolve(), far.image_at(S, counts))
        e2, st = gf.error(1e-3)
        e2s, sts = sf.error(1e-3)
        assert same(e2, e2s) and st == sts and same(e2, far.e2_at(S, Q, counts))
        mean, rgb, _ = gf.denoise()
        means, rgbs, _ = sf.denoise()
        assert same(mean, means) and same(rgb, rgbs)
        gf.write(S[4], Q[4], 4)  # uniform again
        assert gf.count_range() == (4, 4) and gf.accumulate(2) == 6
        assert same(gf.read()[0], golden_data.sums(golden("ref4_32x18x6_d50_s404")))


# ---- 6. the error map -----------------------------------------------------------------------------

def test_error_map_with_counts_below_two(ren, groups):
    p = make_params(**REF4_6)
    g = groups(3)
    g.set_scene(refscenes.ref4(), CAM)
    ren.set_scene(refscenes.ref4(), CAM)
    S, Q = film_ref.prefixes(film_ref.colours(refscenes.ref4(), CAM, p))
    with g.film(p) as gf, ren.film(p) as sf:
        for f in (gf, sf):  # a fresh film has no error map
            with pytest.raises(yk.YkError, match="YK_ERR_INVALID.*two accumulated"):
                f.error(0.0)
        counts = np.full((18, 32), 5, np.uint32)
        counts[1::3] = 1       # every row of entry 1: a uniform entry below two samples
        counts[2::3, :7] = 3   # entry 2 holds two counts
        counts[6, 9] = 0       # entry 0 holds a pixel without samples
        for f in (gf, sf):
            put(f, far.at_counts(S, counts), far.at_counts(Q, counts), counts)
        want = far.e2_at(S, Q, counts)
        for thr2 in (0.0, float(np.median(want[np.isfinite(want)])), float("inf")):
            e2, st = gf.error(thr2)
            e2s, sts = sf.error(thr2)
            assert same(e2, e2s) and same(e2, want), thr2
            assert st == sts and st["max_e2"] == float("inf") and st["samples_done"] == 0, thr2
            assert st["pixels_over"] == int((want > thr2).sum()) and st["pixels"] == 18 * 32
            _, st_only = gf.error(thr2, want_map=False)
            assert st_only == st
        assert same(gf.resolve(), sf.resolve()) and same(gf.resolve(), far.image_at(S, counts))
        # an entry whose pixels all hold no sample: black rows, +inf
        counts[1::3] = 0
        for f in (gf, sf):
            put(f, far.at_counts(S, counts), far.at_counts(Q, counts), counts)
        assert same(gf.resolve(), sf.resolve()) and not gf.resolve()[1::3].any()
        assert same(gf.error(0.0)[0], sf.error(0.0)[0])


# ---- 7. the filters -------------------------------------------------------------------------------

def check_filters(gf, sf, scene, p, sums, sumsq, counts, what, radius, patch):
    """Both filters of the group film against the single film holding the same state and against the
    numpy restatements of the definition."""
    colour = DenoiseParams(radius, patch, 2.0, 1.0, 1e-10)
    before = state(gf)
    mean, rgb, st = gf.denoise(radius=radius, patch=patch)
    means, rgbs, _ = sf.denoise(radius=radius, patch=patch)
    want = fdr.denoise(sums, sumsq, counts, radius=radius, patch=patch)
    assert same(mean, means), f"mean {what}: {int((mean != means).sum())} of {mean.size} values differ from the single film's"
    assert same(mean, want) and same(rgb, rgbs) and same(rgb, fdr.to_rgb8(want)), what
    assert st["features_ms"] == 0.0 and st["filter_ms"] > 0 and st["total_ms"] >= st["filter_ms"]
    assert st["moments_ms"] >= 0 and st["exchange_ms"] >= 0
    gmean, grgb, gst = gf.denoise_guided(colour=colour)
    gmeans, grgbs, _ = sf.denoise_guided(colour=colour)
    gwant = ffr.denoise_guided(sums, sumsq, counts, scene, CAM, p, colour=dict(radius=radius, patch=patch))
    assert same(gmean, gmeans), f"guided mean {what}: {int((gmean != gmeans).sum())} of {gmean.size} values differ"
    assert same(gmean, gwant) and same(grgb, grgbs) and same(grgb, fdr.to_rgb8(gwant)), what
    _, _, again = gf.denoise_guided(colour=colour)
    assert again["features_ms"] == 0.0, what  # the cached pass of this (grid, halo)
    only_mean, none, _ = gf.denoise_guided(colour=colour, want_rgb=False)
    none2, only_rgb, _ = gf.denoise(radius=radius, patch=patch, want_mean=False)
    assert none is None and none2 is None and same(only_mean, gmean) and same(only_rgb, rgb)
    assert all(same(a, b) for a, b in zip(before, state(gf))), f"the filters changed the film {what}"
    return gst


FILTER_CASES = [(3, 5, 1), (5, 5, 1), (4, 10, 3), (1, 5, 1), (3, 0, 2)]


@pytest.mark.parametrize("k,radius,patch", FILTER_CASES,
                         ids=["halo-equals-band", "bands-shorter-than-halo", "halo-13-of-18", "one-entry", "radius-0"])
def test_filters(ren, groups, k, radius, patch):
    p = make_params(**MIXED_16)
    scene = refscenes.mixed12()
    g = groups(k)
    g.set_scene(scene, CAM)
    ren.set_scene(scene, CAM)
    S, Q = mixed_prefixes()
    with g.film(p) as gf, ren.film(p) as sf:
        gf.accumulate(8)
        sf.accumulate(8)
        same_state(gf, sf, "at 8 spp")
        st = check_filters(gf, sf, scene, p, S[8], Q[8], 8, f"uniform {(k, radius, patch)}", radius, patch)
        assert st["features_ms"] > 0  # the first guided call computed the band's feature planes
        # an adaptive (non-uniform) state: half of the pixels four samples further
        sim = far.Sim(film_ref.colours(scene, CAM, p))
        sim.step(-1.0, 8)
        thr2 = sim.threshold2(0.5)
        gf.accumulate_adaptive(thr2, 4)
        sim.step(thr2, 4)
        assert same(gf.counts(), sim.counts) and sim.counts.min() == 8 and sim.counts.max() == 12
        put(sf, sim.sums(), sim.sumsq(), sim.counts)
        check_filters(gf, sf, scene, p, sim.sums(), sim.sumsq(), sim.counts, f"adaptive {(k, radius, patch)}", radius, patch)


def test_filters_four_row_tile_five_entries(ren, groups):
    p = make_params(**MIXED_16, rows=(7, 4, 1))
    scene = refscenes.mixed12()
    g = groups(5)
    g.set_scene(scene, CAM)
    ren.set_scene(scene, CAM)
    S, Q = mixed_prefixes()
    s8, q8 = np.ascontiguousarray(S[8][7:11]), np.ascontiguousarray(Q[8][7:11])
    with g.film(p) as gf, ren.film(p) as sf:
        gf.accumulate(8)
        sf.accumulate(8)
        same_state(gf, sf, "4 rows")
        assert same(gf.read()[0], s8)
        check_filters(gf, sf, scene, p, s8, q8, 8, "4 rows over 5 entries", 5, 1)


@pytest.mark.parametrize("grid", [1, 2])
def test_features(ren, groups, grid):
    p = make_params(**MIXED_16, cols=(3, 21, 1))
    scene = refscenes.mixed12()
    g = groups(3)
    g.set_scene(scene, CAM)
    ren.set_scene(scene, CAM)
    with g.film(p) as gf, ren.film(p) as sf:
        mean, var, ms = gf.features(grid)
        means, vars_, _ = sf.features(grid)
        F, U = ffr.features(scene, CAM, p, grid)
        assert same(mean, means) and same(var, vars_) and same(mean, F) and same(var, U)
        assert ms > 0 and gf.features(grid)[2] == 0.0
        sent = np.full((18, 21, 7), -7.25)
        t = ctypes.c_double(-1.0)
        for bad in (0, 5):  # refused calls write nothing
            assert gf._lib.ykgpu_group_film_features(gf._f, bad, sent.ctypes.data, sent.ctypes.data,
                                                     ctypes.byref(t)) == YK_ERR_INVALID
            assert (sent == -7.25).all() and t.value == -1.0
        assert gf.done == 0 and not gf.counts().any()


def raw_denoise(gf, guided, dp=None, want_mean=True, want_rgb=True):
    """The C call with sentinel-filled outputs; returns (rc, outputs untouched)."""
    rows, wt = gf._shape
    mean, rgb = np.full((rows, wt, 3), -7.25), np.full((rows, wt, 3), 0xA5, np.uint8)
    st = GroupDenoiseStats(-1.0, -1.0, -1.0, -1.0, -1.0)
    args = [gf._f, ctypes.byref(dp) if dp is not None else None]
    if guided:
        args.append(None)
    args += [mean.ctypes.data if want_mean else None, rgb.ctypes.data if want_rgb else None, ctypes.byref(st)]
    rc = (gf._lib.ykgpu_group_film_denoise_guided if guided else gf._lib.ykgpu_group_film_denoise)(*args)
    untouched = bool((mean == -7.25).all() and (rgb == 0xA5).all() and st.total_ms == -1.0 and st.filter_ms == -1.0)
    return rc, untouched


def test_filter_errors_leave_the_outputs_untouched(groups):
    g = groups(3)
    g.set_scene(refscenes.ref4(), CAM)
    p = make_params(**REF4_6)
    S, Q = film_ref.prefixes(film_ref.colours(refscenes.ref4(), CAM, p))
    with g.film(p) as gf:
        for guided in (False, True):
            assert raw_denoise(gf, guided) == (YK_ERR_INVALID, True)  # fresh: count 0
        gf.accumulate(1)
        for guided in (False, True):
            assert raw_denoise(gf, guided) == (YK_ERR_INVALID, True)  # one sample
        with pytest.raises(yk.YkError, match="YK_ERR_INVALID.*two samples"):
            gf.denoise()
        gf.accumulate(3)
        for guided in (False, True):
            assert raw_denoise(gf, guided, DenoiseParams(11, 1, 0.5, 1.0, 1e-10)) == (YK_ERR_INVALID, True)
            assert raw_denoise(gf, guided, DenoiseParams(5, 4, 0.5, 1.0, 1e-10)) == (YK_ERR_INVALID, True)
            assert raw_denoise(gf, guided, DenoiseParams(5, 1, 0.0, 1.0, 1e-10)) == (YK_ERR_INVALID, True)
            assert raw_denoise(gf, guided, want_mean=False, want_rgb=False) == (YK_ERR_INVALID, True)
            assert raw_denoise(gf, guided) == (0, False)  # NULL params: the defaults
        with pytest.raises(yk.YkError, match="YK_ERR_INVALID.*grid"):
            gf.denoise_guided(feat=FeatureParams(5, 0, 2.0, 1.0, 1e-2, 1e-1, 1e-2))
        # one pixel below two samples, in the rows of one entry
        counts = np.full((18, 32), 4, np.uint32)
        counts[5, 7] = 1
        put(gf, far.at_counts(S, counts), far.at_counts(Q, counts), counts)
        for guided in (False, True):
            assert raw_denoise(gf, guided) == (YK_ERR_INVALID, True)
    # a strided P has no neighbours to filter over, however the entries' sub-tiles look
    for kw in (dict(rows=(1, 4, 2)), dict(cols=(3, 5, 2))):
        with g.film(make_params(**REF4_6, **kw)) as gf:
            gf.accumulate(4)
            for guided in (False, True):
                assert raw_denoise(gf, guided) == (YK_ERR_UNSUPPORTED, True), kw
            with pytest.raises(yk.YkError, match="YK_ERR_UNSUPPORTED"):
                gf.denoise()


# ---- 8. checkpoints -------------------------------------------------------------------------------

def test_checkpoints_pass_between_group_and_single_films(ren, groups, tmp_path):
    p = make_params(**MIXED_16)
    scene = refscenes.mixed12()
    h = yk.scene_hash(scene, CAM)
    g = groups(3)
    g.set_scene(scene, CAM)
    ren.set_scene(scene, CAM)
    sim = far.Sim(film_ref.colours(scene, CAM, p))
    path = str(tmp_path / "group.ykfilm")
    with g.film(p) as gf:
        gf.accumulate(4)
        sim.step(-1.0, 4)
        thr2 = sim.threshold2(0.5)
        gf.accumulate_adaptive(thr2, 4)
        sim.step(thr2, 4)
        sums, sumsq, counts = state(gf)
        assert counts.min() != counts.max()
        yk.save_film_counts(path, gf.params, h, counts, sums, sumsq)
    with ren.film(p) as sf:  # ... continued on one context
        assert sf.load(path, h) == 4
        sf.accumulate_adaptive(thr2, 4)
        sim.step(thr2, 4)
        check_against_sim(sf, sim, "continued on one context")
        sf.save(path, h)
    with g.film(p) as gf:  # ... and back on the group
        assert gf.load(path, h) == int(sim.counts.min())
        check_against_sim(gf, sim, "back on the group")
        gf.accumulate_adaptive(thr2, 4)
        sim.step(thr2, 4)
        check_against_sim(gf, sim, "continued on the group")
        gf.accumulate_adaptive(-1.0, 16)
        assert same(gf.read()[0], ren.render_sums(p)) and gf.count_range() == (16, 16)  # the uninterrupted film
        gf.save(path, h)  # (uniform: a v1 file)
        assert yk.load_film(path)[2] == 16


# ---- 9. lifetimes ---------------------------------------------------------------------------------

def test_stale_scene(groups):
    g = groups(2)
    g.set_scene(refscenes.ref4(), CAM)
    with g.film(make_params(**REF4_6)) as gf:
        gf.accumulate(2)
        before = state(gf)
        g.set_scene(refscenes.ref4(), CAM)
        for call in (lambda: gf.accumulate(1), lambda: gf.accumulate_adaptive(-1.0, 1), lambda: gf.features(2),
                     lambda: gf.denoise_guided()):
            with pytest.raises(yk.YkError, match="YK_ERR_INVALID.*scene was set after"):
                call()
        # what only reads the film still works
        assert all(same(a, b) for a, b in zip(before, state(gf)))
        gf.resolve(), gf.error(0.0), gf.denoise()


def test_renders_other_films_and_two_scenes_do_not_disturb(ren, groups):
    g = groups(3)
    p = make_params(**REF4_6)
    other = make_params(40, 22, 5, 50, 7, rng=RNG_XOR128)
    entry = golden("ref4_32x18x6_d50_s404")
    g.set_scene(refscenes.ref4(), CAM)
    ren.set_scene(refscenes.ref4(), CAM)
    other_alone = ren.render(other)
    with g.film(p) as a, g.film(other) as b:
        a.accumulate(2)
        assert same(g.render(other), other_alone)  # a plain group render between two chunks
        b.accumulate(5)  # another group film of the same group
        a.denoise()
        a.accumulate(4)
        b.denoise(radius=2)
        assert same(a.read()[0], golden_data.sums(entry)) and same(a.resolve(), golden_data.rgb(entry))
        assert same(b.resolve(), other_alone)
    # a second scene on the same group, after the first one's films are gone
    arr, cam = yk.build_scene("rtiow5", 0)
    g.set_scene(arr, cam)
    ren.set_scene(arr, cam)
    with g.film(p) as gf:
        gf.accumulate(6)
        assert same(gf.read()[0], ren.render_sums(p)) and same(gf.resolve(), ren.render(p))
