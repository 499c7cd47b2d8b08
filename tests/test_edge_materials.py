"""Conditions on the references alone for the cases of tests/edge_materials.py: the C oracle
(oracle/yk_oracle.c) and the Python restatement (tests/radiance_ref.py) agree on every pixel, the
oracle stays finite and non-negative, and each case reaches the branch it was built for (counted
from the restatement's per-scatter events).  With these held, and the cases' goldens from the
reference harness pinned by tests/test_oracle_golden.py, a failure of
tests/test_gpu_edge_materials.py can only be the kernel's.  Each test prints the counts it
asserts on (pytest -s shows them)."""
import collections
import os

import numpy as np
import pytest

import cast_ref
import edge_materials as em
import golden_data
import radiance_ref as rr
from edge_materials import FP32, FP64, ME, MT, X128

ENGINES = [MT, X128]
ENGINE_IDS = [em.RNG_NAME[r] for r in ENGINES]
ENDS = rr.SKY | rr.ABSORBED | rr.DEPTH | rr.OOD


def counts(events):
    """Counter of (sphere id, front face, branch) over the paths' events."""
    c = collections.Counter()
    for ev in events:
        for e in ev:
            c[e[:3]] += 1
    return c


def total(c, ids=None, front=None, branches=None):
    return sum(n for (i, f, b), n in c.items() if (ids is None or i in ids) and (front is None or f == front)
               and (branches is None or b in branches))


# ---- (a) the references agree, and the oracle stays in range ------------------------------------

@pytest.mark.parametrize("rng", ENGINES, ids=ENGINE_IDS)
@pytest.mark.parametrize("name", em.NAMES)
def test_restatement_equals_the_oracle_on_every_pixel(name, rng):
    recs, _ = em.restated(name, rng)
    p = em.params(name, FP64, rng)
    _, sums, segs = em.oracle(name, FP64, rng)
    assert rr.fold(recs["colour"], p).tobytes() == sums.tobytes()
    assert int(recs["segments"].sum()) == segs
    row =em.draw_counts(name, FP64, rng, rows=(1,)).reshape(-1)
    n = row.size
    assert (recs["words"][n:2 * n] == row).all()  # the words of image row 1 against oracle_lib.sample


@pytest.mark.parametrize("prec,rng", em.MODES, ids=em.MODE_IDS)
@pytest.mark.parametrize("name", em.NAMES)
def test_oracle_is_finite_and_nonnegative(name, prec, rng):
    """Finite sums in all four modes before any kernel sees the case, and no negative pixel sum
    (to_color3b's math::sqrt need not end on one); paths bounce (segments per sample >= 2)."""
    _, sums, segs = em.oracle(name, prec, rng)
    assert np.isfinite(sums).all()
    assert not (sums < 0).any()
    per = segs / em.sample_count(name)
    print(f"{name} {em.PREC_NAME[prec]}-{em.RNG_NAME[rng]}: segments per sample {per:.3f}")
    assert per >= 2.0


def test_scalar_hit_is_the_array_scan():
    """radiance_ref._hit (Python floats) against radiance_ref._hit_scan (cast_ref.scan on
    one-element arrays) on every segment of two image rows of each case: the same bits."""
    n = 0
    for name in em.NAMES:
        sph = em.scene(name)
        p = em.params(name)
        for y, x, s in em.row_samples(name, 5)[:: 1 if name == "matedge24" else 8]:
            o, d, seed, skip = rr.camera_start(em.CAM, p, y, x, s)
            trace = []
            rr.ray_color(sph, cast_ref.extent(sph), o, d, seed, skip, min(p.max_depth, 50), p.t_min, p.rng, trace=trace)
            for so, sd in trace:
                a, b = rr._hit(sph, so, sd, p.t_min), rr._hit_scan(sph, so, sd, p.t_min)
                assert a[1] == b[1] and float(a[0]).hex() == float(b[0]).hex(), (name, y, x, s)
                n += 1
    assert n > 1000


def test_events_change_no_result():
    sph, p = em.scene("matedge24"), em.params("matedge24")
    for y, x, s in em.row_samples("matedge24", 9)[::3]:
        o, d, seed, skip = rr.camera_start(em.CAM, p, y, x, s)
        ev = []
        a = rr.ray_color(sph, cast_ref.extent(sph), o, d, seed, skip, p.max_depth, p.t_min, p.rng)
        b = rr.ray_color(sph, cast_ref.extent(sph), o, d, seed, skip, p.max_depth, p.t_min, p.rng, events=ev)
        assert a == b and len(ev) == a["segments"] - (1 if a["flags"] & rr.SKY else 0)


@pytest.mark.parametrize("name", em.NAMES)
def test_scene_fixture_is_the_python_builder(name):
    """tests/golden/<name>.yks (what the reference harness rendered) holds the builder's bits."""
    sph, cam = golden_data.read_scene_file(os.path.join(golden_data.GOLDEN, name + ".yks"))
    assert [s.as_tuple() for s in sph] == [s.as_tuple() for s in em.scene(name)]
    assert cam.as_tuple() == em.CAM.as_tuple()
    assert len(sph) in (5, 24)
    for s in sph:
        assert s.radius != 0.0 and all(np.isfinite(v) for v in (s.radius, s.fuzz, s.ior, *s.center, *s.albedo))


def test_every_case_and_mode_has_a_reference_golden():
    names = {c["name"] for c in golden_data.manifest()["cases"]}
    for name in em.NAMES:
        _, W, H, spp, depth, seed0 = em.CASES[name]
        base = f"{name}_{W}x{H}x{spp}_d{depth}_s{seed0}"
        want = {base, base + "_f32", base + "_x128"} | ({base + "_f32_x128"} if name == "matedge24" else set())
        assert want <= names, want - names


# ---- (b) matedge24 ------------------------------------------------------------------------------

@pytest.mark.parametrize("rng", ENGINES, ids=ENGINE_IDS)
def test_matedge24_reaches_every_branch(rng):
    """Every sphere scatters but the earlier of the coincident pair (which the tie rule never
    reports: asserted), total internal reflection happens on front faces (ior < 1) and on back
    faces, rays refract through ior 1.0 and nextafter(1, 2), the fuzz-3.0 metal absorbs (and the
    fuzz-1.0 metal with mt19937; with xor128 none of its 32 scatters is absorbed), and the
    negative radii of all three materials scatter."""
    recs, events = em.restated("matedge24", rng)
    c = counts(events)
    ids = {i for (i, _, _) in c}
    print(f"matedge24 {em.RNG_NAME[rng]}:", {k: c[k] for k in sorted(c)})
    assert ids == set(range(24)) - {ME["tied_dielectric"]}
    assert total(c, {ME["tied_lambertian"]}) >= 1
    first = recs["id_first"]
    assert (first == ME["tied_lambertian"]).sum() >= 1 and not (first == ME["tied_dielectric"]).any()
    assert total(c, front=True, branches={"tir"}) >= 1
    assert total(c, front=False, branches={"tir"}) >= 1
    print("  front-face TIR", total(c, front=True, branches={"tir"}), "back-face TIR", total(c, front=False, branches={"tir"}))
    for role in ("ior1", "ior_next1"):
        assert total(c, {ME[role]}, branches={"refracted"}) >= 1, role
    assert total(c, {ME["fuzz3"]}, branches={"absorbed"}) >= 1
    if rng == MT:
        assert total(c, {ME["fuzz1"]}, branches={"absorbed"}) >= 1
    for role in ("shell25", "metal_negr", "lamb_negr"):
        assert total(c, {ME[role]}) >= 1, role
    # a negative radius turns the outward normal inwards: seen from outside it is a back face
    assert total(c, {ME["metal_negr"], ME["lamb_negr"]}, front=False) >= 1
    for role in ("nested15", "mirror_in_0625", "ior17_overlap", "ior01", "ior50", "fuzz0999", "fuzz_tiny", "black",
                 "bright", "negative", "subnormal"):
        assert total(c, {ME[role]}) >= 1, role
    assert (recs["colour"] < 0).any()  # the negative albedo reaches sample colours


def test_matedge24_fuzz_tiny_is_positive_in_double_and_zero_in_float():
    s = em.scene("matedge24")[ME["fuzz_tiny"]]
    assert s.fuzz > 0 and np.float32(s.fuzz) == 0
    assert em.IOR_NEXT1 > 1.0 and np.float32(em.IOR_NEXT1) == 1.0


def test_schlick_r0_of_the_two_faces_differs_in_the_last_bits_only():
    """((1 - 1/n) / (1 + 1/n))^2 and ((1 - n) / (1 + n))^2 are the same number, so the r0 the host
    precomputes for the front face and for the back face differ by rounding alone: at most 2 units
    in the last place over the cases' refractive indices (and 5e-48 at nextafter(1, 2), where both
    are 2^-106).  A kernel that read the wrong face's r0 would change a path only where the
    reflect-or-refract uniform falls inside that gap, about once in 10^16 dielectric hits: no
    image can show it, and none of these tests claims to."""
    iors = sorted({s.ior for name in em.NAMES for s in em.scene(name) if s.material == em.records.MATERIAL_DIELECTRIC})
    assert len(iors) >= 10 and min(iors) == 0.1 and max(iors) == 50.0
    for n in iors:
        inv = 1.0 / n
        f, b = (1 - inv) / (1 + inv), (1 - n) / (1 + n)
        f, b = f * f, b * b
        assert abs(f - b) <= 2 * np.spacing(max(f, b)) or max(f, b) < 2.0 ** -100, n


# ---- (c) room5 ----------------------------------------------------------------------------------

@pytest.mark.parametrize("rng", ENGINES, ids=ENGINE_IDS)
def test_room5_sees_no_sky(rng):
    recs, _ = em.restated("room5", rng)
    ends = collections.Counter((recs["flags"] & ENDS).tolist())
    print(f"room5 {em.RNG_NAME[rng]}: ends", dict(ends), "segments", int(recs["segments"].sum()), "words", int(recs["words"].sum()))
    assert ends[rr.SKY] == 0 and ends[rr.OOD] == 0
    assert ends[rr.ABSORBED] >= 1
    assert ends[rr.DEPTH] == len(recs) - ends[rr.ABSORBED]
    _, sums, _ = em.oracle("room5", FP64, rng)
    assert sums.tobytes() == np.zeros_like(sums).tobytes()  # +0.0, the sign bit clear


@pytest.mark.parametrize("rng", ENGINES, ids=ENGINE_IDS)
def test_room5_leaks_in_float(rng):
    """render<float> is not dark in the room: a point on the radius-40 wall is known to float only
    within a few units of 2^-18, so len2(oc) - r*r is noise of some 1e-4, and a scattered ray that
    leaves the wall at a grazing angle (about one in 400) finds the near root noise / (2 |half_b|)
    above t_min = 0.001: a hit on the wall from outside, after which the path scatters outwards
    and ends on the sky.  That is the reference's own arithmetic (the harness goldens hold the same
    sums), so the FP32 sums are compared with the references like any other case, and +0.0 is
    asserted for FP64 alone."""
    _, sums, segs = em.oracle("room5", FP32, rng)
    lit = int(sums.any(-1).sum())
    print(f"room5 fp32-{em.RNG_NAME[rng]}: pixels with light {lit} of {sums.shape[0] * sums.shape[1]}")
    assert 0 < lit < 20 and segs < 50 * em.sample_count("room5")


# ---- (d) glasswalls5 ----------------------------------------------------------------------------

def test_glasswalls5_meets_glass_at_the_engine_seam():
    """FP64, mt19937: the committed samples hold a dielectric scatter at engine position 224 that
    draws and one that is a total internal reflection (the last position that speculates: the draw
    kept, the draw given back), and the same two at 226 (the first that does not speculate).  The
    restatement is FP64 only, so for FP32 no position is claimed: there the seam is asserted only
    through the draw counts (samples past 227 words)."""
    want = collections.defaultdict(set)
    for y, x, s, pos, kind in em.GLASSWALLS_SEAM:
        want[(y, x, s)].add((pos, kind))
    kinds = collections.Counter()
    for (y, x, s), expect in sorted(want.items()):
        _, ev = em.path("glasswalls5", MT, y, x, s)
        got = {em.seam_kind(e) for e in ev} - {None}
        assert got == expect, (y, x, s)
        for e in ev:
            if em.seam_kind(e):
                kinds[em.seam_kind(e)] += 1
    print("glasswalls5 seam events:", dict(kinds))
    for pos in em.SEAM_POSITIONS:
        for kind in ("drew", "tir"):
            assert kinds[(pos, kind)] >= 1, (pos, kind)


@pytest.mark.parametrize("prec", [FP64, FP32], ids=["fp64", "fp32"])
def test_glasswalls5_draws_past_the_lazy_cursors(prec):
    d = em.draw_counts("glasswalls5", prec, MT)
    print(f"glasswalls5 {em.PREC_NAME[prec]}: samples past 227 words {int((d > 227).sum())}, peak {int(d.max())}")
    assert int((d > 227).sum()) >= 100


# ---- (e) inside_glass5 --------------------------------------------------------------------------

@pytest.mark.parametrize("rng", ENGINES, ids=ENGINE_IDS)
def test_inside_glass5_starts_on_a_back_face(rng):
    recs, events = em.restated("inside_glass5", rng)
    assert all(ev and ev[0][0] == 0 and ev[0][1] is False and em.is_dielectric_event(ev[0]) for ev in events)
    assert (recs["id_first"] == 0).all()
    c = counts(events)
    print(f"inside_glass5 {em.RNG_NAME[rng]}:", {k: c[k] for k in sorted(c)})
    assert total(c, {0}, front=False, branches={"tir"}) >= 1 and total(c, {0}, front=False, branches={"refracted"}) >= 1
