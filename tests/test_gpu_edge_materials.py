"""Edge-material parity on the MI355X: the cases of tests/edge_materials.py through the render
kernels, the radiance and ray queries, a film with its feature pass and a device group, every
result compared byte for byte (no tolerance anywhere) with the CPU oracle, the Python restatement
(radiance_ref), cast_ref and film_features_ref.  tests/test_edge_materials.py holds the conditions
on those references alone, and tests/test_gpu_parity.py::test_golden_case compares the same cases
with the reference harness's goldens.

What the cases reach in the kernels: the dielectric's precomputed 1/ior and Schlick r0 of both
faces at ior 1, nextafter(1, 2), 0.625, 0.1, 1.33, 1.7, 2.5 and 50; total internal reflection on
front and back faces and the speculative word pair given back; a fuzz that is positive in double and
0 in float; fuzz 1 and 3 (absorbed paths); albedos of 0, above 1, negative and subnormal through the
unwind; the hit normal's division by a negative radius on every material; coincident spheres; a
camera inside glass; a room without sky; dielectric hits at engine words 224 and 226."""
import numpy as np
import pytest

import cast_ref
import edge_materials as em
import film_features_ref as ffr
import radiance_ref as rr
import uecraytracing_amd as yk
from edge_materials import FP32, FP64, ME, MT, X128
from uecraytracing_amd import records

pytestmark = pytest.mark.gpu

COUNT_WORK, LINEAR_SCAN = records.FLAG_COUNT_WORK, records.FLAG_LINEAR_SCAN
WORK_ROW = 9  # the image row whose engine words are counted against oracle_lib.sample
RENDER_CASES = [(n, p, r) for n in em.NAMES for p, r in em.MODES]
RENDER_IDS = [f"{n}-{em.PREC_NAME[p]}-{em.RNG_NAME[r]}" for n, p, r in RENDER_CASES]
SCAN_CASES = [(n, p, MT) for n in em.NAMES for p in (FP64, FP32)]
SCAN_IDS = [f"{n}-{em.PREC_NAME[p]}" for n, p, _ in SCAN_CASES]
QUERY_CASES = [(n, r) for n in em.NAMES for r in (MT, X128)]
QUERY_IDS = [f"{n}-{em.RNG_NAME[r]}" for n, r in QUERY_CASES]


@pytest.fixture(scope="module")
def ren():
    r = yk.Renderer(0)
    yield r
    r.close()


def check_render(ren, name, prec, rng, flags):
    """render_sums, render and the segment count against the oracle; the engine words of the
    16x9x2 room5 tile, or of one row of the larger tiles, against oracle_lib.sample's."""
    _, W, H, _, _, _ = em.CASES[name]
    want_rgb, want, segs = em.oracle(name, prec, rng)
    ren.set_scene(em.scene(name), em.CAM)
    p = em.params(name, prec, rng, flags)
    got = ren.render_sums(p)
    st = ren.stats()
    bad = int((got.view(np.uint64) != want.view(np.uint64)).any(-1).sum())
    assert got.tobytes() == want.tobytes(), f"render_sums != oracle on {bad} of {W * H} pixels"
    assert st["segments"] == segs
    np.testing.assert_array_equal(ren.render(p), want_rgb)
    rows = None if name == "room5" else (WORK_ROW,)
    if rows is not None:
        row = ren.render_sums(em.params(name, prec, rng, flags, rows=(WORK_ROW, 1, 1)))
        assert row.tobytes() == want[WORK_ROW:WORK_ROW + 1].tobytes()
        st = ren.stats()
    assert st["work"][5] == int(em.draw_counts(name, prec, rng, rows).sum())
    return got, st


@pytest.mark.parametrize("name,prec,rng", RENDER_CASES, ids=RENDER_IDS)
def test_render_all_modes(ren, name, prec, rng):
    check_render(ren, name, prec, rng, COUNT_WORK)


@pytest.mark.parametrize("name,prec,rng", SCAN_CASES, ids=SCAN_IDS)
def test_linear_scan(ren, name, prec, rng):
    _, st = check_render(ren, name, prec, rng, COUNT_WORK | LINEAR_SCAN)
    assert st["linear_scans"] == st["segments"] > 0


@pytest.mark.parametrize("prec,rng", em.MODES, ids=em.MODE_IDS)
def test_room5_is_dark(ren, prec, rng):
    """No path of the room sees the sky in FP64: every sum is +0.0 (the products of the albedos
    with the depth limit's and the absorptions' black), and the segments are the oracle's.  In FP32
    the reference itself leaks through the radius-40 wall (tests/test_edge_materials.py
    test_room5_leaks_in_float): there the bytes are the oracle's, lit pixels included."""
    _, want, segs = em.oracle("room5", prec, rng)
    ren.set_scene(em.scene("room5"), em.CAM)
    got = ren.render_sums(em.params("room5", prec, rng, COUNT_WORK))
    assert ren.stats()["segments"] == segs
    assert got.tobytes() == want.tobytes()
    if prec == FP64:
        assert got.tobytes() == np.zeros_like(got).tobytes()
    else:
        assert want.any()


def query_samples(name):
    """Every sample of the tile; glasswalls5 (depth 450): the committed seam samples and one row."""
    if name == "glasswalls5":
        return em.SEAM_SAMPLES + em.row_samples(name, WORK_ROW)
    return None


@pytest.mark.parametrize("name,rng", QUERY_CASES, ids=QUERY_IDS)
def test_radiance_queries(ren, name, rng):
    """ykgpu_radiance_rays (the second copy of the shading code, yk_radiance.hpp) over the same
    edges: every field of every record equals the restatement's, and the colours fold to the
    render's sums."""
    samples = query_samples(name)
    want, _ = em.restated(name, rng, samples)
    p = em.params(name, FP64, rng)
    ys, xs, ss = rr.all_samples(p) if samples is None else (np.array(c) for c in zip(*samples))
    rays = rr.camera_rays(em.CAM, p, ys, xs, ss)
    assert yk.camera_sample_rays(em.CAM, p, ys, xs, ss).tobytes() == rays.tobytes()
    ren.set_scene(em.scene(name), em.CAM)
    got = ren.radiance_rays(rays, p.max_depth, p.t_min, p.rng)
    for field in ("colour", "t_first", "id_first", "id_last", "words", "segments", "flags"):
        bad = int((np.atleast_2d(got[field].T != want[field].T)).any(0).sum())
        assert got[field].tobytes() == want[field].tobytes(), f"{field}: {bad} of {len(want)} records differ"
    assert got.tobytes() == want.tobytes()
    sums = ren.render_sums(p)
    if samples is None:
        assert rr.fold(got["colour"], p).tobytes() == sums.tobytes()
    else:
        _, W, _, spp, _, _ = em.CASES[name]
        row = got["colour"][len(em.SEAM_SAMPLES):].reshape(W, spp, 3)
        acc = np.zeros((W, 3), np.float64)
        for s in range(spp):
            acc = acc + row[:, s]
        assert acc.tobytes() == sums[WORK_ROW].tobytes()
        if rng == MT:  # the seam samples: glass met at engine word 224 or 226
            assert (got["words"][:len(em.SEAM_SAMPLES)] >= 224).all()
    if name == "matedge24":
        assert (got["colour"] < 0).any() and (got["id_first"] == ME["tied_lambertian"]).any()
    if name == "inside_glass5":
        assert (got["id_first"] == 0).all()
    if name == "room5":
        assert not (got["flags"] & rr.SKY).any() and (got["flags"] & rr.ABSORBED).any() and not got["colour"].any()


def test_ray_queries_on_matedge24(ren):
    """The first segment of every sample's path through ykgpu_cast_rays: id, t, p, normal and the
    front-face flag equal cast_ref.cast's.  The coincident pair reports the later index, and the
    negative radii report back faces from outside with normals that face the ray."""
    sph = em.scene("matedge24")
    p = em.params("matedge24")
    rays = rr.camera_rays(em.CAM, p, *rr.all_samples(p))
    want = cast_ref.cast(sph, rays["origin"], rays["direction"])
    ren.set_scene(sph, em.CAM)
    for kw in (dict(), dict(linear_scan=True)):
        got = ren.cast_rays(rays["origin"], rays["direction"], **kw)
        bad = int((got.view(np.uint64).reshape(-1, 8) != want.view(np.uint64).reshape(-1, 8)).any(1).sum())
        assert got.tobytes() == want.tobytes(), f"{kw}: {bad} of {len(want)} records differ"
    assert (want["id"] == ME["tied_lambertian"]).sum() >= 8 and not (want["id"] == ME["tied_dielectric"]).any()
    for role in ("metal_negr", "lamb_negr"):
        rec = want[want["id"] == ME[role]]
        assert len(rec) >= 8 and (rec["flags"] == records.HIT_HIT).all(), role  # a hit, not a front face
        d = rays["direction"][want["id"] == ME[role]]
        assert ((d * rec["normal"]).sum(1) < 0).all(), role
    assert set(np.unique(want["id"][want["flags"] != 0]).tolist()) >= set(range(24)) - {
        ME["tied_dielectric"], ME["nested15"], ME["mirror_in_0625"], ME["shell25"], ME["negative"]}


def test_film_and_features_on_matedge24(ren):
    """A film of target 4 accumulated as 1 + 3 holds the one-shot sums; the feature pass at grid 2
    equals film_features_ref: the albedo planes carry the out-of-range albedos and (1, 1, 1) for
    the dielectrics, the normal planes the negative-radius normals."""
    sph = em.scene("matedge24")
    p = em.params("matedge24")
    _, want, _ = em.oracle("matedge24", FP64, MT)
    ren.set_scene(sph, em.CAM)
    with ren.film(p) as film:
        assert film.accumulate(1) == 1 and film.accumulate(3) == 4
        sums, _, done = film.read()
        assert done == 4 and sums.tobytes() == want.tobytes()
        mean, var, _ = film.features(2)
    F, U = ffr.features(sph, em.CAM, p, 2)
    assert mean.tobytes() == F.tobytes(), f"{int((mean != F).sum())} of {F.size} feature means differ"
    assert var.tobytes() == U.tobytes(), f"{int((var != U).sum())} of {U.size} feature variances differ"
    for role in ("bright", "subnormal", "black", "metal_negr", "lamb_negr"):  # a pixel wholly on each
        assert (F[..., 0:3] == np.array(tuple(sph[ME[role]].albedo))).all(-1).any(), role
    # a pixel wholly on the ior-2.5 ball: albedo (1, 1, 1) and a hit (a miss has depth 0)
    o, d = cast_ref.pixel_rays(em.CAM, p.image_width, p.image_height)
    centre = cast_ref.cast(sph, o, d)["id"].reshape(p.image_height, p.image_width)
    on_glass = (centre == ME["ior25"]) & (U[..., 0:3] == 0).all(-1) & (F[..., 6] > 0)
    assert on_glass.any() and (F[on_glass][:, 0:3] == 1.0).all()
    for role in ("metal_negr", "lamb_negr"):  # the normal faces the camera: n.z > 0 at the sphere's middle
        on = (centre == ME[role]) & (U[..., 0:3] == 0).all(-1)
        assert on.any() and (F[on][:, 5] > 0).all(), role


def test_group_on_matedge24(ren):
    p = em.params("matedge24")
    ren.set_scene(em.scene("matedge24"), em.CAM)
    want = ren.render(p)
    np.testing.assert_array_equal(want, em.oracle("matedge24", FP64, MT)[0])
    with yk.Group([0, 0, 0]) as g:
        g.set_scene(em.scene("matedge24"), em.CAM)
        np.testing.assert_array_equal(g.render(p), want)
