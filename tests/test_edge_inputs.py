"""Conditions on the CPU oracle alone for the cases of tests/edge_inputs.py: each case reaches the
guard it was chosen for, and the oracle itself stays inside its number format there.  With these
held, a failure of tests/test_gpu_edge_inputs.py can only be the kernel's."""
import numpy as np
import pytest

import edge_inputs as ei
import oracle_lib
import refscenes
from edge_inputs import FP32, FP64, MT, X128


@pytest.mark.parametrize("prec,rng", ei.DEEP_CASES, ids=ei.DEEP_IDS)
def test_deep_case_runs_past_the_second_twist(prec, rng):
    """walls2 16x9x4 at depth 450: samples draw more than 1248 words (the third twist of the
    scratch engine, idx == 0 in mt_slow) in both precisions, FP32 more than 624 (its second)."""
    d = ei.draw_counts(refscenes.walls2(), refscenes.reference_camera(), ei.deep_params(prec, rng))
    assert d.size == 576
    assert d.max() > 1248
    if prec == FP32:
        assert (d > 624).any()
    if rng == MT:
        m = ei.DEEP_MEASURED[(prec, rng)]
        assert int(d.max()) == m["peak"]
        assert int((d > 1248).sum()) == m["gt1248"]
        if "gt1872" in m:
            assert int((d > 1872).sum()) == m["gt1872"]
        if "gt624" in m:
            assert int((d > 624).sum()) == m["gt624"]


def test_expected_twists_is_the_scratch_engine_schedule():
    """One twist at draw 227 (word index 227 is the first the lazy cursors cannot serve), then one
    whenever the word index is a multiple of 624."""
    def twists(n):  # words 0 .. n-1 drawn
        return sum(1 for j in range(n) if j == 227 or (j > 227 and j % 624 == 0))
    for n in (0, 1, 227, 228, 624, 625, 1248, 1249, 1872, 1873, 1960):
        assert ei.expected_twists(n) == twists(n), n


@pytest.mark.parametrize("prec,name,k", ei.SCALE_CASES, ids=ei.SCALE_IDS)
def test_scaled_scene_keeps_its_paths_in_the_oracle(prec, name, k):
    sph, cam, p = ei.scale_case(prec, name, k)
    _, sums, segs = ei.oracle(("scale", prec, name, k), sph, cam, p)
    assert np.isfinite(sums).all()
    samples = ei.SCALE_W * ei.SCALE_H * ei.SCALE_SPP
    assert segs / samples >= ei.SCALE_MIN_SEGMENTS_PER_SAMPLE, segs / samples


def test_scaling_is_exact():
    sph, cam = ei.golden_scene("final48")
    for k in (-240, -21, 24, 240):
        s2, c2 = ei.scaled(*ei.scaled(sph, cam, k), -k)
        assert [s.as_tuple() for s in s2] == [s.as_tuple() for s in sph]
        assert c2.as_tuple() == cam.as_tuple()
        assert ei.t_min_for(k) == 0.001 * min(1.0, 2.0 ** k)


def test_f32_cases_sit_on_both_sides_of_the_host_guard():
    """The FP32 k lists cross ykgpu_set_scene's guard (rmin >= 2^-20, origin bound <= 2^20) on
    both sides for both scenes."""
    for name in ("rtiow5", "final48"):
        inside = [ei.f32_tree_in_range(*ei.scale_case(FP32, n, k)[:2]) for p, n, k in ei.SCALE_CASES
                  if p == FP32 and n == name]
        assert any(inside) and not all(inside), name
        assert not inside[0] and not inside[-1], name  # out of range at both ends of the list


@pytest.mark.parametrize("prec,k", ei.DIR_CASES, ids=ei.DIR_IDS)
def test_direction_scale_in_the_oracle(prec, k):
    """A shorter primary direction (k < 0) changes no hit: the sums are the k = 0 sums bit for bit.
    (A longer one shrinks the roots below t_min: those cases stand on their own.)"""
    sph, cam, p = ei.dir_case(prec, k)
    _, sums, _ = ei.oracle(("dir", prec, k), sph, cam, p)
    assert np.isfinite(sums).all()
    if k < 0:
        sph0, cam0, p0 = ei.dir_case(prec, 0)
        _, sums0, _ = ei.oracle(("dir", prec, 0), sph0, cam0, p0)
        assert sums.tobytes() == sums0.tobytes()


@pytest.mark.parametrize("axis", ei.PLANAR_AXES)
def test_planar_cameras_have_an_exactly_zero_component(axis):
    cam = ei.planar_camera(axis)
    comp = 1 if axis == "y" else 0
    for u in (0.0, 0.3, 1.0):
        for v in (0.0, 0.7, 1.0):
            d = ((cam.lower_left_corner[comp] + u * cam.horizontal[comp]) + v * cam.vertical[comp]) \
                - cam.origin[comp]
            assert d == 0.0
            assert np.signbit(d) == (axis == "x-negzero")


@pytest.mark.parametrize("prec,name,axis", ei.PLANAR_CASES, ids=ei.PLANAR_IDS)
def test_planar_case_hits_something_in_the_oracle(prec, name, axis):
    sph, cam, p = ei.planar_case(prec, name, axis)
    _, sums, segs = ei.oracle(("planar", prec, name, axis), sph, cam, p)
    assert np.isfinite(sums).all()
    assert segs > ei.PLANAR_W * ei.PLANAR_H * ei.PLANAR_SPP  # some paths bounce


@pytest.mark.parametrize("rng,word,seed,y", ei.CLAMP_CASES, ids=ei.CLAMP_IDS)
def test_clamp_seeds_draw_a_word_that_rounds_to_one(rng, word, seed, y):
    """The committed seeds: the engine's first (second) word is >= 0xFFFFFF80, so
    generate_canonical<float> reaches 1.0f and clamps; clamp_params gives that seed to sample 0 of
    pixel (0, y)."""
    draw = oracle_lib.xor128 if rng == X128 else oracle_lib.mt19937
    assert draw(seed, word + 1)[word] >= ei.CLAMP_WORD
    assert np.float32(draw(seed, word + 1)[word]) == np.float32(2.0 ** 32)
    p = ei.clamp_params(rng, seed, y)
    assert (p.seed0 + y * p.image_width * p.samples_per_pixel) & 0xFFFFFFFF == seed


def test_xor128_closed_form_reaches_all_ones():
    assert oracle_lib.xor128(ei.xor128_seed_for_word(0), 1)[0] == 0xFFFFFFFF
    assert oracle_lib.xor128(ei.xor128_seed_for_word(1), 2)[1] == 0xFFFFFFFF
