"""Sky blocks on the MI355X: the blocks of a tile whose camera rays can hit nothing
leave the path pipeline and yk_sky_samples renders them.  Every image here is compared with the CPU
oracle byte for byte (RGB8) and bit for bit (the float64 sums): the sky kernel's samples must be the
path kernel's, its fold the ordered reduce's, across launches, calls, tiles and a changed scene.

72x40 at 6 spp: 45 blocks with partial ones at the bottom edge, two launches (4 + 2).  The named
scenes have few sky blocks at this size (final48 without a lens: 3; with its lens, and rtiow5: none —
tests/test_sky_blocks.py says why), so the same calls also run on final48 seen by a camera pitched up,
where 33 of the 45 blocks are sky and the other 12 hold the silhouette and the partial bottom row,
with and without a lens.
"""
import os

import numpy as np
import pytest

import golden_data
import oracle_lib
import refscenes
import sky_blocks_lib as sbl
import uecraytracing_amd as yk
from uecraytracing_amd import tiles
from uecraytracing_amd.records import FLAG_COUNT_WORK, PRECISION_FP32, make_params

pytestmark = pytest.mark.gpu

ROOT = sbl.ROOT
W, H, SPP, DEPTH = 72, 40, 6, 50
FILES = {"rtiow5": os.path.join(ROOT, "uecraytracing_amd", "scenes", "rtiow5.yks"),
         "final48": os.path.join(ROOT, "tests", "golden", "final48.yks")}
CASES = [("rtiow5", 0.0), ("rtiow5", 0.05), ("final48", 0.0), ("final48", 0.05), ("pitched", 0.0), ("pitched", 0.05)]
_oracle = {}


def scene(name, lens):
    if name == "pitched":
        return list(yk.read_scene(FILES["final48"])[0]), sbl.look_at((13, 2, 3), (0, 4.5, 0), (0, 1, 0), 40.0, 16 / 9,
                                                                     2 * lens, 10.0)
    if name == "all_sky":
        s, c = sbl.all_sky_scene()
        return s, sbl.with_lens(c, lens)
    if name == "no_sky":
        s, c = sbl.no_sky_scene()
        return s, sbl.with_lens(c, lens)
    s, c = yk.read_scene(FILES[name])
    return list(s), sbl.with_lens(c, lens)


def oracle(name, lens, p):
    """(rgb, sums) of the CPU oracle, computed once per scene and params."""
    key = (name, lens, bytes(p))
    if key not in _oracle:
        s, c = scene(name, lens)
        rgb, sums, _, _ = oracle_lib.render(s, c, p, want_sums=True)
        _oracle[key] = (rgb, sums)
    return _oracle[key]


def same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def ren():
    r = yk.Renderer(0)
    yield r
    r.close()


# sky blocks of each case at 72x40 (the classifier's count, tests/test_sky_blocks.py): the first three
# cases run the whole order, as before; the others must take the culled path
SKY_BLOCKS = {("rtiow5", 0.0): 0, ("rtiow5", 0.05): 0, ("final48", 0.05): 0, ("final48", 0.0): 3,
              ("pitched", 0.0): 33, ("pitched", 0.05): 33}


@pytest.mark.parametrize("name,lens", CASES, ids=[f"{n}-lens{l}" for n, l in CASES])
def test_image_and_sums_equal_the_oracle(ren, name, lens, tmp_path):
    s, c = scene(name, lens)
    ren.set_scene(s, c)
    p = make_params(W, H, SPP, DEPTH, 404)
    rgb, sums = oracle(name, lens, p)
    got = ren.render(p)
    st = ren.stats()
    assert st["launches"] == 2 and st["samples"] == W * H * SPP
    np.testing.assert_array_equal(got, rgb)
    assert same_bits(ren.render_sums(p), sums)
    # which path ran: the counting instance never culls, and a culled call needs other bytes (fewer
    # start records and colours, the sky slots' buffers) than the same call over the whole order
    ren.render(make_params(W, H, SPP, DEPTH, 404, flags=FLAG_COUNT_WORK))
    culled = ren.stats()["call_bytes"] != st["call_bytes"]
    assert culled == (SKY_BLOCKS[(name, lens)] > 0)
    path = str(tmp_path / "scene.txt")
    sbl.write_scene(path, s, c)
    grid = sbl.classify(sbl.build_driver(tmp_path), path, sbl.geometry(W, H))
    assert sum(grid["flags"]) == SKY_BLOCKS[(name, lens)]


@pytest.mark.parametrize("name,lens", [("final48", 0.0), ("pitched", 0.05)], ids=["final48", "pitched-lens"])
def test_back_to_back_calls(ren, name, lens):
    """Three calls enqueued without a wait between them and one synced call: four equal images."""
    import torch
    ren.set_scene(*scene(name, lens))
    p = make_params(W, H, SPP, DEPTH, 404)
    rgb, _ = oracle(name, lens, p)
    outs = [torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda:0") for _ in range(3)]
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    for o in outs:
        ren.render_async(p, o.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    for o in outs:
        np.testing.assert_array_equal(o.cpu().numpy(), rgb)
    np.testing.assert_array_equal(ren.render(p), rgb)


@pytest.mark.parametrize("lens", (0.0, 0.05))
def test_all_sky_and_no_sky_calls(ren, lens):
    p = make_params(W, H, SPP, DEPTH, 404)
    ren.set_scene(*scene("all_sky", lens))
    rgb, sums = oracle("all_sky", lens, p)
    np.testing.assert_array_equal(ren.render(p), rgb)
    st = ren.stats()
    assert st["launches"] == 0 and st["kernel_ms"] == 0 and st["warmup_ms"] == 0, "no path launch in an all-sky call"
    assert st["samples"] == W * H * SPP and st["mt_fallbacks"] == 0
    assert same_bits(ren.render_sums(p), sums)
    # ... and a path call right after it on the same context
    ren.set_scene(*scene("no_sky", lens))
    rgb, sums = oracle("no_sky", lens, p)
    np.testing.assert_array_equal(ren.render(p), rgb)
    st = ren.stats()
    assert st["launches"] == 2 and st["kernel_ms"] > 0 and st["warmup_ms"] > 0
    assert same_bits(ren.render_sums(p), sums)
    # every sample went through the path kernel: the counting instance, which never culls, counts
    # the same launches and at least a segment per sample
    ren.render(make_params(W, H, SPP, DEPTH, 404, flags=FLAG_COUNT_WORK))
    stc = ren.stats()
    assert stc["launches"] == st["launches"] and stc["launch_spp"] == st["launch_spp"]
    assert stc["segments"] >= W * H * SPP


@pytest.mark.parametrize("name,lens", [("final48", 0.0), ("pitched", 0.05)], ids=["final48", "pitched-lens"])
def test_two_way_tiles(ren, name, lens):
    ren.set_scene(*scene(name, lens))
    for rank in (0, 1):
        for kw in ({"rows": tiles.tile_rows(rank, 2, H)}, {"cols": tiles.tile_cols(rank, 2, W)}):
            p = make_params(W, H, SPP, DEPTH, 404, **kw)
            rgb, sums = oracle(name, lens, p)
            np.testing.assert_array_equal(ren.render(p), rgb)
            assert same_bits(ren.render_sums(p), sums)


@pytest.mark.parametrize("name,lens", [("rtiow5", 0.0), ("pitched", 0.05)], ids=["rtiow5", "pitched-lens"])
def test_progressive_film_equals_one_render(ren, name, lens):
    """Two film passes (samples 0-2, then 3-5) == one 6-spp render == the oracle."""
    ren.set_scene(*scene(name, lens))
    p = make_params(W, H, SPP, DEPTH, 404)
    rgb, sums = oracle(name, lens, p)
    one = ren.render_sums(p)
    with ren.film(p) as film:
        assert film.accumulate(3) == 3 and film.accumulate(3) == 6
        fs, _, done = film.read()
        assert done == 6 and same_bits(fs, one) and same_bits(fs, sums)
        np.testing.assert_array_equal(film.resolve(), rgb)


def test_set_scene_invalidates_the_blocks(ren):
    """The same spheres, then the camera pitched up: the second image is the new camera's."""
    p = make_params(W, H, SPP, DEPTH, 404)
    for name, lens in (("final48", 0.0), ("pitched", 0.0), ("final48", 0.0), ("all_sky", 0.0), ("pitched", 0.05)):
        ren.set_scene(*scene(name, lens))
        rgb, sums = oracle(name, lens, p)
        assert same_bits(ren.render_sums(p), sums), name
        np.testing.assert_array_equal(ren.render(p), rgb)


def test_counting_and_fp32_calls_are_unchanged(ren):
    """The counting instance and the FP32 mode keep the whole processing order: the oracle's image
    and segment count, and the reference-generated FP32 golden."""
    s, c = scene("pitched", 0.05)
    ren.set_scene(s, c)
    p = make_params(W, H, SPP, DEPTH, 404, flags=FLAG_COUNT_WORK)
    rgb, _, segments, _ = oracle_lib.render(s, c, p)
    np.testing.assert_array_equal(ren.render(p), rgb)
    st = ren.stats()
    assert st["segments"] == segments and st["samples"] == W * H * SPP and st["launches"] == 2
    np.testing.assert_array_equal(ren.render(make_params(W, H, SPP, DEPTH, 404)), rgb)  # (and the culled call)
    e = next(k for k in golden_data.manifest()["cases"] if k["name"] == "mixed12_96x54x16_d50_s404_f32")
    ren.set_scene(refscenes.mixed12(), refscenes.reference_camera())
    got = ren.render(make_params(e["W"], e["H"], e["spp"], e["depth"], e["seed0"], precision=PRECISION_FP32))
    np.testing.assert_array_equal(got, golden_data.rgb(e))
