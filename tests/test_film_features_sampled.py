"""The sampled feature pass' host side (no device): the numpy yardstick (film_features_sampled_ref)
pinned to what already pins the library — its start rays to the host's yk_camera_sample_ray byte for
byte, its per-sample hits to the first segment radiance_ref.ray_color records — its edge rules, the
tuning table of DESIGN.md §6.8 against the committed profile, and the new record, defaults and
entry points.  The GPU tests (test_gpu_film_features_sampled.py) compare the library with this
yardstick byte for byte.
"""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import cast_ref
import edge_inputs
import film_denoise_ref as fdr
import film_features_ref as ffr
import film_features_sampled_ref as fsr
import film_ref
import radiance_ref as rr
import refscenes
import uecraytracing_amd as yk
from uecraytracing_amd import records
from uecraytracing_amd.records import D3, Camera, make_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TUNE = json.load(open(os.path.join(ROOT, "profiles", "r19_features_sampled_tune.json")))
CAM = refscenes.reference_camera()
KEY = 0x1234567890ABCDEF
START_CASES = {
    "mt-counter": dict(),
    "xor128-counter": dict(rng=records.RNG_XOR128),
    "mt-keyed": dict(seed_mode=records.SEED_RANDOM_DEVICE, seed_key=KEY),
    "xor128-keyed": dict(rng=records.RNG_XOR128, seed_mode=records.SEED_RANDOM_DEVICE, seed_key=KEY),
    "mt-seed-wraps": dict(seed0=4294967000),
}


def params(w, h, spp, seed0=404, **kw):
    return make_params(w, h, spp, 50, seed0, **kw)


@pytest.mark.parametrize("case", sorted(START_CASES))
def test_start_rays_are_the_librarys_camera_sample_rays(case):
    sph, cam = edge_inputs.golden_scene("final48")
    assert cam.lens_radius > 0
    kw = dict(START_CASES[case])
    p = params(16, 9, 3, seed0=kw.pop("seed0", 404), **kw)
    o, d, _, _ = fsr.first_hits(sph, cam, p, 3)
    ys, xs, ss = rr.all_samples(p)
    want = yk.camera_sample_rays(cam, p, ys, xs, ss)
    assert o.reshape(-1, 3).tobytes() == np.ascontiguousarray(want["origin"]).tobytes()
    assert d.reshape(-1, 3).tobytes() == np.ascontiguousarray(want["direction"]).tobytes()


@pytest.mark.parametrize("name,cam", [("final48", None), ("ref4", CAM)])
def test_hits_are_the_first_segment_of_ray_color(name, cam):
    if cam is None:
        sph, cam = edge_inputs.golden_scene(name)
    else:
        sph = refscenes.SCENES[name]()
    sph = list(sph)
    p = params(16, 9, 2)
    o, d, hit, t = fsr.first_hits(sph, cam, p, 2)
    E = cast_ref.extent(sph)
    for y in range(9):
        for x in range(16):
            for s in range(2):
                so, sd, seed, skip = rr.camera_start(cam, p, y, x, s)
                trace = []
                rec = rr.ray_color(sph, E, so, sd, seed, skip, trace=trace)
                assert trace[0] == (tuple(o[y, x, s]), tuple(d[y, x, s]))
                if rec["id_first"] == rr.NO_ID:
                    assert hit[y, x, s] == -1
                else:
                    assert (hit[y, x, s], t[y, x, s]) == (rec["id_first"], rec["t_first"])


def test_one_sample_has_no_variance_and_folds_are_in_sample_order():
    sph, cam = edge_inputs.golden_scene("final48")
    p = params(16, 9, 4)
    F1, U1, st = fsr.features(sph, cam, p, 1)
    assert not U1.any() and st["samples"] == 16 * 9
    o, d, hit, t = fsr.first_hits(sph, cam, p, 3)
    f = fsr.channels(sph, o, d, hit, t)
    assert F1.tobytes() == f[:, :, 0].tobytes()  # (x / 1.0 is x)
    F3, U3, st3 = fsr.features(sph, cam, p, 3)
    s = (f[:, :, 0] + f[:, :, 1]) + f[:, :, 2]
    q = (f[:, :, 0] * f[:, :, 0] + f[:, :, 1] * f[:, :, 1]) + f[:, :, 2] * f[:, :, 2]
    assert F3.tobytes() == (s / 3.0).tobytes()
    var = (q - (s * s) / 3.0) / (3.0 * (3.0 - 1.0))
    assert U3.tobytes() == np.where(var > 0.0, var, 0.0).tobytes() and (U3 >= 0).all() and U3.any()
    assert st3 == dict(samples=16 * 9 * 3, hits=int((hit >= 0).sum()))


def test_a_camera_pointed_at_nothing_gives_the_miss_channels():
    c = CAM
    away = Camera(c.origin, D3(-c.lower_left_corner[0], 50.0, 1.0), c.horizontal, c.vertical, c.lens_u, c.lens_v, 0.0)
    p = params(16, 9, 2)
    F, U, st = fsr.features(refscenes.ref4(), away, p, 2)
    assert st["hits"] == 0 and not U.any()
    assert (F == np.array([1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0])).all()


def test_a_pinhole_camera_differs_from_the_pinhole_pass_by_jitter_only():
    """No lens: the sampled rays leave the camera's origin like the sub-rays, only elsewhere in the pixel."""
    p = params(16, 9, 4)
    o, _, _, _ = fsr.first_hits(refscenes.ref4(), CAM, p, 4)
    assert (o == np.array(tuple(CAM.origin))).all()
    F, _, _ = fsr.features(refscenes.ref4(), CAM, p, 4)
    G, _ = ffr.features(refscenes.ref4(), CAM, p, 2)
    assert F.tobytes() != G.tobytes() and np.abs(F[..., 0:3] - G[..., 0:3]).max() <= 1.0


def scene_of(case):
    if case.startswith("final"):
        arr, cam = yk.build_scene("final", 42)
        if case == TUNE["control"]:
            cam = Camera(cam.origin, cam.lower_left_corner, cam.horizontal, cam.vertical, cam.lens_u, cam.lens_v, 0.0)
        return list(arr), cam
    return refscenes.SCENES[case](), CAM


def chosen():
    c = TUNE["chosen"]
    return (dict(radius=5, patch=1, k2=c["colour_k2"]),
            dict(k2=c["k2_f"], alpha=1.0, tau_albedo=c["tau_albedo"], tau_normal=c["tau_normal"], tau_depth=c["tau_depth"]),
            c["n"])


@pytest.mark.parametrize("case", sorted(TUNE["table"]))
def test_tuning_table_is_the_committed_profile(case):
    spec, geo = TUNE["table"][case], TUNE["cases"][case]
    w, h, spp = geo["width"], geo["height"], geo["spp"]
    scene, cam = scene_of(case)
    assert (cam.lens_radius > 0) == (case == "final")
    truth = fdr.truth(scene, cam, w, h)
    p = params(w, h, spp)
    S, Q = film_ref.prefixes(film_ref.colours(scene, cam, p))
    colour, feat, n = chosen()
    assert spec["n_used"] == min(n, spp)
    got = dict(raw=fdr.mse(S[spp] / float(spp), truth), colour_only=fdr.mse(fdr.denoise(S[spp], Q[spp], spp), truth),
               guided_pinhole_g2=fdr.mse(ffr.denoise_guided(S[spp], Q[spp], spp, scene, cam, p), truth),
               guided_sampled=fdr.mse(fsr.denoise_guided(S[spp], Q[spp], spp, scene, cam, p, min(n, spp), colour=colour,
                                                          feat=feat), truth))
    print(case, {k: repr(v) for k, v in got.items()})
    for k, v in got.items():
        assert abs(v - spec[k]) <= 1e-9 * spec[k], k
    assert abs(got["guided_sampled"] / got["guided_pinhole_g2"] - spec["sampled_over_pinhole"]) <= 1e-9 * spec["sampled_over_pinhole"]


def test_record_defaults_and_exports():
    S = records.SampledFeaturesStats
    assert ctypes.sizeof(S) == 32
    assert (S.ms.offset, S.samples.offset, S.hits.offset, S.redo_pixels.offset, S.reserved.offset) == (0, 8, 16, 24, 28)
    assert ctypes.sizeof(records.FeatureParams) == 48  # (unchanged)
    dp, fp, n = yk.guided_sampled_defaults()
    colour, feat, want_n = chosen()
    assert dp.as_dict() == dict(ffr.COLOUR_DEFAULTS, **colour) and n == want_n
    assert fp.as_dict() == dict(ffr.FEATURE_DEFAULTS, **feat) and fp.reserved == 0
    if not TUNE["a_sampled_point_beats_the_pinhole_pair"]:
        pair = yk.guided_defaults()
        assert (dp.as_dict(), fp.as_dict(), n) == (pair[0].as_dict(), pair[1].as_dict(), 16)
    assert yk.guided_defaults()[1].as_dict() == ffr.FEATURE_DEFAULTS  # (yk_guided_defaults stays)
    lib = yk.load_library()
    assert lib.yk_guided_sampled_defaults(None, None, None) == 1
    only = ctypes.c_uint32(0)
    assert lib.yk_guided_sampled_defaults(None, None, ctypes.byref(only)) == 0 and only.value == n
    header = open(os.path.join(ROOT, "include", "ykgpu.h")).read()
    for name in ("yk_guided_sampled_defaults", "ykgpu_film_features_sampled", "ykgpu_film_denoise_guided_sampled",
                 "ykgpu_group_film_features_sampled", "ykgpu_group_film_denoise_guided_sampled"):
        assert name in yk.EXPORTS and hasattr(lib, name) and name + "(" in header, name
    assert "typedef struct yk_sampled_features_stats {" in header
    assert "#define YKGPU_ABI_VERSION 11u" in header and lib.ykgpu_abi_version() == yk.ABI_VERSION == 11
    assert lib.ykgpu_film_features_sampled(None, 2, None, None, None) == 1 and b"null film" in lib.ykgpu_last_error()
    assert lib.ykgpu_film_denoise_guided_sampled(None, None, None, 2, None, None, None) == 1
    assert b"null film" in lib.ykgpu_last_error()
    for name in ("SampledFeaturesStats", "guided_sampled_defaults"):
        assert name in yk.__all__
    for cls in (yk.Film, yk.GroupFilm):
        assert hasattr(cls, "features_sampled") and hasattr(cls, "denoise_guided_sampled")


def run_cli(*args):
    return subprocess.run([yk.CLI_PATH, *args], capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("args", [["--feature-samples", "4", "a.png"], ["--denoise", "--feature-samples", "4", "a.png"],
                                  ["--aov", "p", "--feature-samples", "0", "a.png"],
                                  ["--aov", "p", "--feature-samples", "257", "--spp", "512", "a.png"],
                                  ["--aov", "p", "--feature-samples", "x", "a.png"],
                                  ["--denoise-features", "--feature-samples", "9", "--spp", "8", "a.png"]])
def test_cli_reports_bad_feature_samples(args):
    r = run_cli(*args)
    assert r.returncode == 2
    assert r.stderr.startswith("raytrace: ") and "see --help" in r.stderr


def test_cli_help_names_the_option():
    assert "--feature-samples arg" in run_cli("--help").stdout
