"""The fallbacks no input reaches in the product build, run on the MI355X through two test variants of
the library (uecraytracing_amd/csrc/Makefile TESTVARIANTS) and compared byte for byte, with no
tolerance, with the CPU references and with the product library's output.

* abl/libykgpu_skylazy8.so (-DYK_SKY_LAZY_FORCE=8): yk_sky_samples lists a pixel for yk_sky_redo as
  soon as the first lens candidate of one of its samples is rejected (four jitter words and one try of
  four), instead of after ~55 rejections in a row.  The redo's whole engines, the sums carried between
  the two kernels from launch to launch in both directions, the list shared by them and cleared
  between launches and calls, and the sky-only call all run, on the scenes of test_gpu_sky_blocks.py.
  The path has no counter, so test_the_inputs_reach_the_redo proves on the CPU that they do.
* abl/libykgpu_qstack2.so (-DYK_QUERY_STACK_FORCE=2): the checked per-lane stack of the four query
  kernels (cast, radiance, gather, sampled features) holds 2 entries instead of the tree's proven
  depth, so a lane whose traversal needs more drops its partial (best, best_id) and takes the ordered
  scan, beside lanes of the same wave that stay in the tree.  2 is the smallest capacity that leaves
  both kinds of lane in one launch on these inputs; share of the cast's rays that took the scan,
  observed on the MI355X with 2, 3, 4 and 5 entries: 61.2%, 20.4%, 5.4%, 0.9% (the product: none).

Each library runs in a fresh child process (tests/fallbacks_child.py, selected by YKGPU_LIB_OVERRIDE),
one process per group of calls and library; the children's files are shared by the tests of a group.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cast_ref
import film_features_sampled_ref as fsr
import gather_ref
import radiance_ref as rr
import refscenes
import sky_blocks_lib as sbl
import test_gpu_sky_blocks as sky_cases
import uecraytracing_amd as yk
from uecraytracing_amd import records, tiles
from uecraytracing_amd.records import make_params

gpu = pytest.mark.gpu  # (every test but the CPU proof that the inputs reach the sky redo)

W, H, SPP, DEPTH = sky_cases.W, sky_cases.H, sky_cases.SPP, sky_cases.DEPTH
LENS = 0.05
MT, X128 = records.RNG_MT19937, records.RNG_XOR128
LIBS = {"product": "libykgpu.so", "skylazy8": os.path.join("abl", "libykgpu_skylazy8.so"),
        "qstack2": os.path.join("abl", "libykgpu_qstack2.so")}


def run_child(group, name, folder):
    """Runs the group's calls with library `name`; returns (arrays, statistics)."""
    lib = os.path.join(yk.LIB_DIR, LIBS[name])
    assert os.path.exists(lib), f"{lib}: built by uecraytracing_amd/csrc/Makefile (all)"
    env = dict(os.environ, YKGPU_LIB_OVERRIDE=lib)
    pr = subprocess.run([sys.executable, os.path.join(sbl.ROOT, "tests", "fallbacks_child.py"), group, str(folder)],
                        env=env, capture_output=True, text=True, timeout=240)
    assert pr.returncode == 0, pr.stderr[-2000:]
    with open(os.path.join(str(folder), "stats.json")) as f:
        stats = json.load(f)
    with np.load(os.path.join(str(folder), "out.npz")) as z:
        return {k: z[k] for k in z.files}, stats


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def differing(a, b):
    """how many records (or pixels) of two equally shaped arrays differ, for a failure's message"""
    a, b = (np.ascontiguousarray(v).view(np.uint8).reshape(len(v), -1) for v in (a, b))
    return f"{int((a != b).any(1).sum())} of {len(a)} differ"


# =====================================================================================================
# the sky blocks' whole-engine path
# =====================================================================================================

@pytest.fixture(scope="module")
def sky_runs(tmp_path_factory):
    return {name: run_child("sky", name, tmp_path_factory.mktemp("sky_" + name)) for name in ("product", "skylazy8")}


def sky_params(key):
    """(scene name, lens, params) of a call of the child's sky group"""
    if key.startswith("rows"):
        return "pitched", LENS, make_params(W, H, SPP, DEPTH, 404, rows=tiles.tile_rows(int(key[4:]), 2, H))
    if key.startswith("cols"):
        return "pitched", LENS, make_params(W, H, SPP, DEPTH, 404, cols=tiles.tile_cols(int(key[4:]), 2, W))
    if key.startswith("spp"):
        return "pitched", LENS, make_params(W, H, int(key[3:]), DEPTH, 404)
    p = make_params(W, H, SPP, DEPTH, 404)
    return {"whole": ("pitched", LENS, p), "lens0": ("pitched", 0.0, p), "all_sky": ("all_sky", LENS, p),
            "no_sky": ("no_sky", LENS, p)}[key]


def check_sky_call(sky_runs, key):
    """The call's image and sums in the variant: the oracle's and the product library's."""
    name, lens, p = sky_params(key)
    rgb, sums = sky_cases.oracle(name, lens, p)
    (got, st), (prod, pst) = sky_runs["skylazy8"], sky_runs["product"]
    assert same(prod[key + "_rgb"], rgb) and same(prod[key + "_sums"], sums), f"{key}: the product library"
    assert same(got[key + "_rgb"], rgb), f"{key} rgb: {differing(got[key + '_rgb'].reshape(-1, 3), rgb.reshape(-1, 3))}"
    assert same(got[key + "_sums"], sums), f"{key} sums: {differing(got[key + '_sums'].reshape(-1, 3), sums.reshape(-1, 3))}"
    assert same(got[key + "_rgb"], prod[key + "_rgb"]) and same(got[key + "_sums"], prod[key + "_sums"])
    # the statistics: the redo counts a fallback only past mt19937's 227 lazy words
    for k in ("launches", "launch_spp", "samples", "mt_fallbacks"):
        assert st[key][k] == pst[key][k], (key, k, st[key], pst[key])
    assert st[key]["samples"] == p.row_count * p.tile_width() * p.samples_per_pixel
    return st[key]


def test_the_inputs_reach_the_redo(tmp_path):
    """On the CPU: camera_start's skip is the words a start drew, four for the jitter and four per
    lens candidate, so skip > 8 is a rejected first candidate, which the variant lists.  Over the
    pixels of the blocks the classifier flags, more pixels are listed than one round of the redo's 64
    threads, and with the two launches of 4 + 2 samples each of the four ways a pixel can move between
    yk_sky_samples and yk_sky_redo occurs: listed in the first launch only (the second launch's
    yk_sky_samples continues from the redo's sums), in the second only (the redo continues from
    yk_sky_samples' sums and stores the pixel), in both, in neither."""
    s, c = sky_cases.scene("pitched", LENS)
    p = make_params(W, H, SPP, DEPTH, 404)
    path = str(tmp_path / "scene.txt")
    sbl.write_scene(path, s, c)
    g = sbl.geometry(W, H)
    grid = sbl.classify(sbl.build_driver(tmp_path), path, g)
    assert sum(grid["flags"]) == 33
    classes = {(a, b): 0 for a in (False, True) for b in (False, True)}
    for j in range(grid["by"]):
        for i in range(grid["bx"]):
            if grid["flags"][j * grid["bx"] + i]:
                xs, ys = sbl.block_pixels(g, grid, i, j)
                for y in ys:
                    for x in xs:
                        rej = [rr.camera_start(c, p, y, x, k)[3] > 8 for k in range(SPP)]
                        classes[(any(rej[:4]), any(rej[4:]))] += 1
    print("sky pixels listed in (launch 0, launch 1):", classes)
    assert sum(classes.values()) == 33 * 64
    assert sum(n for k, n in classes.items() if any(k)) > 64
    assert all(n >= 1 for n in classes.values()), classes


@gpu
def test_sky_redo_whole_image(sky_runs):
    st = check_sky_call(sky_runs, "whole")
    assert st["launches"] == 2  # 4 + 2: the carry crosses a launch


@gpu
def test_sky_redo_two_way_tiles(sky_runs):
    for rank in (0, 1):
        check_sky_call(sky_runs, f"rows{rank}")
        check_sky_call(sky_runs, f"cols{rank}")


@gpu
def test_sky_redo_back_to_back_calls(sky_runs):
    """Three calls enqueued without a wait between them and a synced one: four equal images, so the
    list is cleared and refilled between launches and calls."""
    rgb, _ = sky_cases.oracle("pitched", LENS, make_params(W, H, SPP, DEPTH, 404))
    for name in ("product", "skylazy8"):
        got = sky_runs[name][0]
        for key in ("async0_rgb", "async1_rgb", "async2_rgb", "async_synced_rgb"):
            assert same(got[key], rgb), f"{name} {key}: {differing(got[key].reshape(-1, 3), rgb.reshape(-1, 3))}"


@gpu
def test_sky_only_call_with_a_redo_then_a_path_call(sky_runs):
    st = check_sky_call(sky_runs, "all_sky")
    assert st["launches"] == 0 and st["kernel_ms"] == 0 and st["warmup_ms"] == 0, "no path launch in an all-sky call"
    st = check_sky_call(sky_runs, "no_sky")
    assert st["launches"] == 2 and st["kernel_ms"] > 0


@gpu
def test_sky_control_without_a_lens(sky_runs):
    check_sky_call(sky_runs, "lens0")


@gpu
@pytest.mark.parametrize("spp", [1, 5])
def test_sky_redo_launch_splits_off_the_walks_interleave(sky_runs, spp):
    """1 and 5 samples: launches whose sample count is no multiple of the seed walk's interleave."""
    st = check_sky_call(sky_runs, f"spp{spp}")
    assert st["launches"] == (1 if spp == 1 else 2)


# =====================================================================================================
# stack overflow to the ordered scan in the query kernels
# =====================================================================================================

def final_scene():
    arr, cam = yk.read_scene(os.path.join(yk.SCENE_DIR, "final_seed42.yks"))
    return list(arr), cam


def make_query_inputs():
    """The children's inputs, made on the CPU: nothing the code under test computed goes into them."""
    sph, cam = final_scene()
    assert len(sph) == 485
    inp = {}
    inp["pixel_o"], inp["pixel_d"] = cast_ref.pixel_rays(cam, 64, 36)
    for name, rng in (("mt", MT), ("x128", X128)):
        inp["rad_small_" + name] = rr.camera_rays(cam, make_params(16, 9, 4, 50, 404, rng=rng),
                                                  *rr.all_samples(make_params(16, 9, 4, 50, 404)))
        inp["rad_big_" + name] = rr.camera_rays(cam, make_params(64, 36, 2, 50, 404, rng=rng),
                                                *rr.all_samples(make_params(64, 36, 2, 50, 404)))
    hits, _ = gather_ref.first_hits(sph, cam, 16, 9)
    assert len(hits) >= 64
    seeds = (5000 + 7919 * np.arange(64, dtype=np.uint64)).astype(np.uint32)
    inp["points"] = gather_ref.make_points(hits["p"][:64], hits["normal"][:64], seeds)
    inp["leaf_o"], inp["leaf_d"] = cast_ref.pixel_rays(refscenes.reference_camera(), 16, 9)
    return inp


@pytest.fixture(scope="module")
def query_inputs():
    return make_query_inputs()


@pytest.fixture(scope="module")
def query_runs(tmp_path_factory, query_inputs):
    runs = {}
    for name in ("product", "qstack2"):
        folder = tmp_path_factory.mktemp("query_" + name)
        np.savez(os.path.join(str(folder), "inputs.npz"), **query_inputs)
        runs[name] = run_child("query", name, folder)
    return runs


def any_hit_records(want):
    """any-hit by its definition: YK_HIT_HIT exactly when closest mode reports a hit, else as a miss"""
    out = np.zeros(len(want), records.HIT_DTYPE)
    out["id"] = records.NO_HIT_ID
    out["flags"] = np.where(want["flags"] == records.HIT_OUT_OF_DOMAIN, want["flags"], want["flags"] & records.HIT_HIT)
    return out


@gpu
def test_cast_overflow_takes_the_scan(query_runs, query_inputs):
    """The pixel rays of 64x36 and the path kernel's traced rays of 16x9x4, closest and any-hit.
    Observed on the MI355X with 2 entries: scan_rays / rays = 2330 / 3808 = 61.2% in both modes."""
    sph, _ = final_scene()
    (got, st), (prod, pst) = query_runs["qstack2"], query_runs["product"]
    assert same(got["traced"], prod["traced"]) and len(got["traced"]) > 16 * 9 * 4
    o = np.concatenate([query_inputs["pixel_o"], got["traced"][:, 0:3]])
    d = np.concatenate([query_inputs["pixel_d"], got["traced"][:, 3:6]])
    want = cast_ref.cast(sph, o, d)
    for mode, ref in (("closest", want), ("any", any_hit_records(want))):
        key = "cast_" + mode
        print(key, "scan_rays / rays:", st[key]["scan_rays"], "/", st[key]["rays"], "product:", pst[key]["scan_rays"])
        assert same(prod[key], ref), f"product {mode}: {differing(prod[key], ref)}"
        assert same(got[key], ref), f"{mode}: {differing(got[key], ref)}"
        assert same(got[key], prod[key])
        assert st[key]["rays"] == pst[key]["rays"] == len(o) and st[key]["out_of_domain"] == pst[key]["out_of_domain"] == 0
        assert st[key]["hits"] == pst[key]["hits"] == int(((want["flags"] & records.HIT_HIT) != 0).sum())
        assert 0 < st[key]["scan_rays"] < st[key]["rays"], st[key]  # tree lanes and overflow lanes in one launch
        assert pst[key]["scan_rays"] == 0


@gpu
@pytest.mark.parametrize("engine", ["mt", "x128"])
def test_radiance_overflow_takes_the_scan(query_runs, query_inputs, engine):
    """The camera starts of 16x9x4 against radiance_ref record for record, and of 64x36x2 against the
    product library, both engines: a path's overflowing segments take the scan, its others the tree.
    Observed on the MI355X with 2 entries, scan_segments / segments: 758 / 1504 = 50.4% (16x9x4) and
    6289 / 12455 = 50.5% (64x36x2) with mt19937, 811 / 1601 = 50.7% and 6858 / 13210 = 51.9% with
    xor128."""
    sph, _ = final_scene()
    rng = MT if engine == "mt" else X128
    (got, st), (prod, pst) = query_runs["qstack2"], query_runs["product"]
    small, big = f"rad_small_{engine}", f"rad_big_{engine}"
    want = rr.radiance(sph, query_inputs[small], 50, records.T_MIN, rng)
    assert same(prod[small], want), f"product: {differing(prod[small], want)}"
    assert same(got[small], want), f"{small}: {differing(got[small], want)}"
    assert same(got[big], prod[big]), f"{big}: {differing(got[big], prod[big])}"
    for key in (small, big):
        print(key, "scan_segments / segments:", st[key]["scan_segments"], "/", st[key]["segments"])
        assert st[key]["rays"] == pst[key]["rays"] == len(query_inputs[key])
        assert st[key]["segments"] == pst[key]["segments"] == int(got[key]["segments"].sum())
        assert st[key]["words"] == pst[key]["words"] and st[key]["mt_fallbacks"] == pst[key]["mt_fallbacks"]
        assert 0 < st[key]["scan_segments"] < st[key]["segments"], st[key]
        assert pst[key]["scan_segments"] == 0


@gpu
def test_gather_overflow_takes_the_scan(query_runs, query_inputs):
    sph, _ = final_scene()
    (got, st), (prod, pst) = query_runs["qstack2"], query_runs["product"]
    assert same(got["gather64"], prod["gather64"]), differing(got["gather64"], prod["gather64"])
    assert st["gather64"]["rays"] == pst["gather64"]["rays"] == 64 * 16
    assert st["gather64"]["open"] == pst["gather64"]["open"] == int(got["gather64"]["open"].sum()) > 0
    want = gather_ref.gather(sph, query_inputs["points"][:8], 4)
    assert same(prod["gather8"], want)
    assert same(got["gather8"], want), differing(got["gather8"], want)


@gpu
def test_sampled_features_overflow_takes_the_scan(query_runs):
    sph, cam = final_scene()
    F, U, want = fsr.features(sph, cam, make_params(32, 18, 8, 50, 404), 8)
    (got, st), (prod, pst) = query_runs["qstack2"], query_runs["product"]
    for name, out in (("product", prod), ("qstack2", got)):
        assert same(out["feat_mean"], F), f"{name} mean: {int((out['feat_mean'] != F).sum())} of {F.size} values differ"
        assert same(out["feat_var"], U), f"{name} variance: {int((out['feat_var'] != U).sum())} of {U.size} values differ"
    assert same(got["feat_mean"], prod["feat_mean"]) and same(got["feat_var"], prod["feat_var"])
    assert st["feat"]["hits"] == pst["feat"]["hits"] == want["hits"] and 0 < want["hits"] < want["samples"]
    assert st["feat"]["samples"] == pst["feat"]["samples"] == want["samples"]
    assert st["feat"]["redo_pixels"] == pst["feat"]["redo_pixels"] == 0


@gpu
@pytest.mark.parametrize("n", [1, 2])
def test_cast_of_a_one_leaf_and_a_one_node_tree(query_runs, query_inputs, n):
    """One sphere: the FP64 tree holds one sphere per leaf, so the root is a leaf code, which the
    forced capacity must leave in the tree: no node is visited, nothing is pushed, nothing overflows.
    Two spheres: one node over two leaves, at most one entry pushed.  In both only the rays the slab
    test cannot serve (a zero direction component: the image's middle row) take the scan."""
    sph = refscenes.ref4()[:n]
    o, d = query_inputs["leaf_o"], query_inputs["leaf_d"]
    want = cast_ref.cast(sph, o, d)
    hits = int(((want["flags"] & records.HIT_HIT) != 0).sum())
    zero = int((d == 0).any(1).sum())
    assert 0 < hits < len(want) and 0 < zero < len(want)
    for name in ("product", "qstack2"):
        got, st = query_runs[name]
        for mode, ref in (("closest", want), ("any", any_hit_records(want))):
            key = f"leaf{n}_{mode}"
            assert same(got[key], ref), f"{name} {mode}: {differing(got[key], ref)}"
            assert st[key]["rays"] == len(want) and st[key]["hits"] == hits
            assert st[key]["scan_rays"] == zero, (name, st[key])
            assert st[key]["node_visits"] == (0 if n == 1 else len(want) - zero), (name, st[key])
            assert st[key]["sphere_tests"] > 0
