"""Edge-input parity on the MI355X: the cases of tests/edge_inputs.py, every one bit for bit
against the CPU oracle at the same input (no tolerance anywhere).

Every kernel proof of exactness is paired with a range guard and a fallback; these cases sit on
both sides of the guards: the scratch mt19937 engine past its second twist, scenes and ray
directions scaled by powers of two across the fast-division, square-root, slab and float-tree
ranges, rays with an exactly zero direction component, engine words that round to 1.0f, and
degenerate image shapes.  tests/test_edge_inputs.py holds the conditions on the oracle alone.

One function per family.  Unless stated otherwise a case asserts, separately: the production
instance's sums and bytes equal the oracle's; the counting instance's tree path (flags=1) and its
linear scan (flags=3) each equal the oracle's sums, and each other."""

import numpy as np
import pytest

import edge_inputs as ei
import refscenes
import uecraytracing_amd as yk
from edge_inputs import FP32, FP64, X128

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ren():
    r = yk.Renderer(0)
    yield r
    r.close()


def with_flags(p, flags):
    q = type(p).from_buffer_copy(p)
    q.flags = flags
    return q


def check_case(ren, key, sph, cam, p):
    """The three assertions of a case (module docstring).  Returns (oracle sums, the tree
    render's sums, its stats)."""
    want_rgb, want, _ = ei.oracle(key, sph, cam, p)
    ren.set_scene(sph, cam)
    got = ren.render_sums(p)
    assert got.tobytes() == want.tobytes(), "render_sums != oracle"
    np.testing.assert_array_equal(ren.render(p), want_rgb)
    tree = ren.render_sums(with_flags(p, 1))
    st = ren.stats()
    lin = ren.render_sums(with_flags(p, 3))
    assert lin.tobytes() == want.tobytes(), "linear scan (flags=3) != oracle"
    assert tree.tobytes() == want.tobytes(), "tree path (flags=1) != oracle"
    assert tree.tobytes() == lin.tobytes(), "tree path != linear scan"
    return want, tree, st


@pytest.mark.parametrize("prec,rng", ei.DEEP_CASES, ids=ei.DEEP_IDS)
def test_deep_paths(ren, prec, rng):
    """walls2 16x9x4 at depth 450: third and fourth twists of the scratch mt19937 engine (FP32:
    its second too), the attenuation-id spill past 200 entries, and the work counters the
    roofline model reads against the oracle's per-sample draw counts."""
    sph, cam, p = refscenes.walls2(), refscenes.reference_camera(), ei.deep_params(prec, rng)
    _, _, st = check_case(ren, ("deep", prec, rng), sph, cam, p)
    draws = ei.draw_counts(sph, cam, p)
    assert st["work"][5] == int(draws.sum())
    if rng == X128:
        assert st["work"][7] == 0
        assert st["mt_fallbacks"] == 0
    else:
        assert st["work"][7] == sum(ei.expected_twists(int(n)) for n in draws.ravel())
        assert st["mt_fallbacks"] == int((draws > 227).sum())


@pytest.mark.parametrize("prec,name,k", ei.SCALE_CASES, ids=ei.SCALE_IDS)
def test_scaled_scenes(ren, prec, name, k):
    """The scene and camera times 2^k, t_min with them: both sides of the fast division's and the
    square root's ranges, of the slab reciprocal's, and of float's own range for the FP64 tree's
    planes; and both sides of the host guards (ykgpu_set_scene) that hand a scene whose float images
    leave float's safe range to the linear scan."""
    sph, cam, p = ei.scale_case(prec, name, k)
    _, _, st = check_case(ren, ("scale", prec, name, k), sph, cam, p)
    in_range = ei.f32_tree_in_range(sph, cam) if prec == FP32 else ei.f64_tree_in_range(sph, cam)
    assert st["segments"] > 0
    if in_range:
        assert st["linear_scans"] < st["segments"]
    else:
        assert st["linear_scans"] == st["segments"]


@pytest.fixture(scope="module")
def dir_k0(ren):
    """The GPU's own sums at k = 0, once per precision."""
    out = {}
    for prec in (FP64, FP32):
        sph, cam, p = ei.dir_case(prec, 0)
        ren.set_scene(sph, cam)
        out[prec] = ren.render_sums(p)
        out[prec].setflags(write=False)
    return out


@pytest.mark.parametrize("prec,k", ei.DIR_CASES, ids=ei.DIR_IDS)
def test_direction_scale(ren, dir_k0, prec, k):
    """Primary rays 2^k times as long over unit-scale geometry: |d|^2 across the FP32 cone's range
    and the divisions', (float)d beyond float's range for the FP64 slabs."""
    sph, cam, p = ei.dir_case(prec, k)
    _, tree, _ = check_case(ren, ("dir", prec, k), sph, cam, p)
    if k < 0:
        assert tree.tobytes() == dir_k0[prec].tobytes(), "sums changed with the direction's length"


@pytest.mark.parametrize("prec,name,axis", ei.PLANAR_CASES, ids=ei.PLANAR_IDS)
def test_planar_cameras(ren, prec, name, axis):
    """Every primary ray (and the mirror reflections that stay in the plane) has a direction
    component that is exactly +0.0 or -0.0: the slab test's 1/0."""
    sph, cam, p = ei.planar_case(prec, name, axis)
    check_case(ren, ("planar", prec, name, axis), sph, cam, p)


@pytest.mark.parametrize("rng,word,seed,y", ei.CLAMP_CASES, ids=ei.CLAMP_IDS)
def test_f32_canonical_clamp(ren, rng, word, seed, y):
    """generate_canonical<float> reaching 1.0f in the sample's first (second) jitter draw: the
    clamp in the seed-walk kernel's start (mt19937) and in the render kernel's own (xor128)."""
    sph, cam, p = refscenes.ref4(), refscenes.reference_camera(), ei.clamp_params(rng, seed, y)
    check_case(ren, ("clamp", rng, word), sph, cam, p)


@pytest.mark.parametrize("case", ei.SHAPE_CASES, ids=ei.SHAPE_IDS)
def test_image_shapes(ren, case):
    """One-pixel-wide, one-pixel-high, one-sample and depth-0 / depth-1 images, and widths and
    heights past 2^12, 2^16 and 10^6 (the pixel coordinate divisions and their magic numbers)."""
    prec, shape = case[0], case[1:]
    sph, cam, p = refscenes.ref4(), refscenes.reference_camera(), ei.shape_params(prec, *shape)
    want, _, _ = check_case(ren, ("shape",) + case, sph, cam, p)
    if shape[3] == 0:
        assert not want.any()  # max_depth 0: every sample is black
