"""The film features' host side (no device): the numpy yardstick (film_features_ref) against the
definition of include/ykgpu.h "film features", and the new records, entry points and options.

The GPU tests (test_gpu_film_features.py) compare ykgpu_film_features and ykgpu_film_denoise_guided
with the yardstick byte for byte.  Here the yardstick is pinned to the specification: the feature pass
against a second, scalar restatement in plain Python floats; its stated cases (ties, the face-forward
normal, a miss, one sub-ray, the ignored lens); the guided filter's identity with the colour filter
when every group is switched off; and the mean squared errors against 1024-spp images at the shipped
defaults (figures of tools/features_tune.py, profiles/r10_features_tune.json and DESIGN.md §6.4,
reproduced to 1e-9 relative)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import film_denoise_ref as fdr
import film_features_ref as ffr
import film_ref
import oracle_lib
import refscenes
import uecraytracing_amd as yk
from uecraytracing_amd import records
from uecraytracing_amd.records import D3, Camera, dielectric, lambertian, make_params

CAM = refscenes.reference_camera()
INF = float("inf")
OFF = dict(tau_albedo=INF, tau_normal=INF, tau_depth=INF)


def state(scene, cam, width, height, n):
    return film_ref.prefixes(film_ref.colours(scene, cam, make_params(width, height, n, 50, 404)))


def test_all_groups_off_is_the_colour_filter_byte_for_byte():
    p = make_params(16, 9, 4, 50, 404)
    S, Q = film_ref.prefixes(film_ref.colours(refscenes.ref4(), CAM, p))
    for params in (dict(fdr.DEFAULTS), dict(fdr.DEFAULTS, radius=2, patch=0, k2=0.25)):
        want = fdr.denoise(S[4], Q[4], 4, **params)
        got = ffr.denoise_guided(S[4], Q[4], 4, refscenes.ref4(), CAM, p, colour=params, feat=OFF)
        assert got.tobytes() == want.tobytes()
    # ... and a finite tau changes it (the weight is a bound, not a no-op)
    got = ffr.denoise_guided(S[4], Q[4], 4, refscenes.ref4(), CAM, p, colour=dict(fdr.DEFAULTS))
    assert got.tobytes() != fdr.denoise(S[4], Q[4], 4).tobytes()


def scalar_features(spheres, cam, p, g):
    """The definition once more, one pixel and one Python float operation at a time."""
    dot = lambda a, b: (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]  # noqa: E731
    W, H = p.image_width, p.image_height
    o, llc, hor, ver = (tuple(getattr(cam, n)) for n in ("origin", "lower_left_corner", "horizontal", "vertical"))
    ys, xs = film_ref.tile_rows(p), film_ref.tile_cols(p)
    F, U = np.zeros((len(ys), len(xs), 7)), np.zeros((len(ys), len(xs), 7))
    for r, y in enumerate(ys):
        for c, x in enumerate(xs):
            s, q = [0.0] * 7, [0.0] * 7
            for i in range(g):
                for j in range(g):
                    a, b = (float(j) + 0.5) / float(g), (float(i) + 0.5) / float(g)
                    u, v = (float(x) + a) / float(W), (float(H - y - 1) + b) / float(H)
                    d = tuple(((llc[k] + hor[k] * u) + ver[k] * v) - o[k] for k in range(3))
                    closest, rec = INF, None
                    for sp in spheres:
                        ctr, radius = tuple(sp.center), sp.radius
                        oc = tuple(o[k] - ctr[k] for k in range(3))
                        aa, half_b = dot(d, d), dot(oc, d)
                        cc = dot(oc, oc) - radius * radius
                        disc = half_b * half_b - aa * cc
                        if disc < 0:
                            continue
                        sq = oracle_lib.newton_sqrt(disc)
                        root = (-half_b - sq) / aa
                        if root < p.t_min or closest < root:
                            root = (-half_b + sq) / aa
                            if root < p.t_min or closest < root:
                                continue
                        closest = root
                        pt = tuple(o[k] + d[k] * root for k in range(3))
                        outward = tuple((pt[k] - ctr[k]) / radius for k in range(3))
                        nrm = outward if dot(d, outward) < 0 else tuple(-w for w in outward)
                        alb = (1.0, 1.0, 1.0) if sp.material == records.MATERIAL_DIELECTRIC else tuple(sp.albedo)
                        rec = alb + nrm + (root,)
                    f = rec if rec is not None else (1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0)
                    for k in range(7):
                        s[k] = s[k] + f[k]
                        q[k] = q[k] + (f[k] * f[k])
            G = float(g * g)
            for k in range(7):
                F[r, c, k] = s[k] / G
                if g >= 2:
                    var = (q[k] - (s[k] * s[k]) / G) / (G * (G - 1.0))
                    U[r, c, k] = var if var > 0.0 else 0.0
    return F, U


@pytest.mark.parametrize("g", [1, 2])
def test_numpy_pass_equals_the_scalar_restatement(g):
    p = make_params(16, 9, 4, 50, 404)
    F, U = ffr.features(refscenes.ref4(), CAM, p, g)
    F2, U2 = scalar_features(refscenes.ref4(), CAM, p, g)
    assert F.tobytes() == F2.tobytes() and U.tobytes() == U2.tobytes()
    assert F.shape == (9, 16, 7) and (U > 0).any() == (g == 2)


def test_scalar_restatement_on_a_strided_sub_tile_and_the_shell():
    p = make_params(16, 9, 4, 50, 404, rows=(1, 4, 2), cols=(3, 5, 2))
    F, U = ffr.features(ffr.shell(), CAM, p, 2)
    F2, U2 = scalar_features(ffr.shell(), CAM, p, 2)
    assert F.tobytes() == F2.tobytes() and U.tobytes() == U2.tobytes()
    whole, _ = ffr.features(ffr.shell(), CAM, make_params(16, 9, 4, 50, 404), 2)
    assert F.tobytes() == np.ascontiguousarray(whole[1:9:2, 3:13:2]).tobytes()  # per pixel, in image coordinates


def test_ties_go_to_the_later_index():
    scene = refscenes.dupes()  # six coincident spheres, tuple indices 1..6
    F, _ = ffr.features(scene, CAM, make_params(16, 9, 4, 50, 404), 1)
    centre = F[4, 8]
    assert tuple(centre[0:3]) == tuple(scene[6].albedo) != tuple(scene[1].albedo)
    assert centre[6] > 0 and centre[5] > 0.9  # (the sphere in front of the camera, facing it)


def test_the_normal_faces_the_ray_on_a_negative_radius_sphere():
    p = make_params(16, 9, 4, 50, 404)
    neg, _ = ffr.features([dielectric((0, 0, -1), -0.5, 1.5)], CAM, p, 1)
    pos, _ = ffr.features([dielectric((0, 0, -1), 0.5, 1.5)], CAM, p, 1)
    hit = pos[:, :, 6] > 0
    assert hit.any() and not hit.all()
    # outward = (p - c) / r points inwards for r < 0, and the face-forward rule flips it back
    assert neg.tobytes() == pos.tobytes()
    assert (pos[hit][:, 5] > 0).all() and (pos[hit][:, 0:3] == 1.0).all()
    # from inside a sphere the normal is -outward: it points at the centre, towards the camera
    inside, _ = ffr.features([lambertian((0, 0, 0), 2.0, (0.5, 0.5, 0.5))], CAM, p, 1)
    assert (inside[:, :, 5] > 0).all() and (inside[:, :, 6] > 0).all()
    # the shell scene: a dielectric record's own albedo is not the feature
    F, _ = ffr.features(ffr.shell(), CAM, p, 1)
    assert (F[4, 12, 0:3] == 1.0).all() and F[4, 12, 6] > 0


def test_a_miss_and_one_sub_ray():
    p = make_params(16, 9, 4, 50, 404)
    F, U = ffr.features(refscenes.ref4(), CAM, p, 1)
    assert F[0, 0].tolist() == [1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0]  # the sky
    assert not U.any()  # g = 1: no variance
    F2, U2 = ffr.features(refscenes.ref4(), CAM, p, 2)
    assert F2[0, 0].tolist() == F[0, 0].tolist() and not U2[0, 0].any()
    assert (U2 >= 0).all() and U2[3, 5].all()  # (a pixel on the red sphere's silhouette)


def test_the_lens_is_ignored():
    p = make_params(16, 9, 4, 50, 404)
    c = CAM
    lens = Camera(c.origin, c.lower_left_corner, c.horizontal, c.vertical, D3(1, 0, 0), D3(0, 1, 0), 0.25)
    a, b = ffr.features(refscenes.mixed12(), lens, p, 2), ffr.features(refscenes.mixed12(), CAM, p, 2)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


# scene, width, height, samples: raw MSE, colour-only MSE (film_denoise_ref at its defaults), guided MSE
MSE_CASES = {
    "ref4": (48, 27, 8, 0.0014187406884441007, 0.0005264189871792214, 0.00033298232496816),
    "lambert3": (48, 27, 8, 0.0022838461150109573, 0.0006679471614424755, 0.000366482512543167),
    "mixed12": (64, 36, 16, 0.0007955148701554881, 0.0003978491064184538, 0.00035616137756611576),
    "final": (96, 54, 16, 0.000925827401330671, 0.0006910507527082543, 0.0006016653249104724),
}


@pytest.mark.parametrize("case", sorted(MSE_CASES))
def test_guided_beats_colour_only_at_the_shipped_defaults(case):
    w, h, n, raw_spec, base_spec, guided_spec = MSE_CASES[case]
    if case == "final":
        arr, cam = yk.build_scene("final", 42)  # the thin-lens camera: the features ignore it
        scene = list(arr)
        assert cam.lens_radius > 0
    else:
        scene, cam = refscenes.SCENES[case](), CAM
    truth = fdr.truth(scene, cam, w, h)
    S, Q = state(scene, cam, w, h, n)
    p = make_params(w, h, n, 50, 404)
    raw = fdr.mse(S[n] / float(n), truth)
    base = fdr.mse(fdr.denoise(S[n], Q[n], n), truth)
    guided = fdr.mse(ffr.denoise_guided(S[n], Q[n], n, scene, cam, p), truth)
    print(case, "raw", repr(raw), "colour-only", repr(base), "guided", repr(guided), "ratio", guided / base)
    assert guided < base < raw
    for got, spec in ((raw, raw_spec), (base, base_spec), (guided, guided_spec)):
        assert abs(got - spec) <= 1e-9 * spec
    assert abs(guided / base - guided_spec / base_spec) <= 1e-9 * (guided_spec / base_spec)


def test_records_defaults_and_exports():
    P, S = records.FeatureParams, records.GuidedStats
    assert ctypes.sizeof(P) == 48 and ctypes.sizeof(S) == 32
    assert (P.grid.offset, P.reserved.offset, P.k2.offset, P.alpha.offset, P.tau_albedo.offset, P.tau_normal.offset,
            P.tau_depth.offset) == (0, 4, 8, 16, 24, 32, 40)
    assert (S.features_ms.offset, S.moments_ms.offset, S.filter_ms.offset, S.total_ms.offset) == (0, 8, 16, 24)
    dp, fp = yk.guided_defaults()
    assert dp.as_dict() == ffr.COLOUR_DEFAULTS and fp.as_dict() == ffr.FEATURE_DEFAULTS and fp.reserved == 0
    assert yk.denoise_defaults().as_dict() == fdr.DEFAULTS  # (ykgpu_film_denoise's own defaults stay)
    lib = yk.load_library()
    assert lib.yk_guided_defaults(None, None) == 1
    only = records.FeatureParams()
    assert lib.yk_guided_defaults(None, ctypes.byref(only)) == 0 and only.as_dict() == ffr.FEATURE_DEFAULTS
    header = open(os.path.join(os.path.dirname(yk.PKG_DIR), "include", "ykgpu.h")).read()
    for name in ("yk_guided_defaults", "ykgpu_film_features", "ykgpu_film_denoise_guided"):
        assert name in yk.EXPORTS and hasattr(lib, name) and name + "(" in header, name
    assert "typedef struct yk_feature_params {" in header and "typedef struct yk_guided_stats {" in header
    assert "#define YKGPU_ABI_VERSION 11u" in header and lib.ykgpu_abi_version() == yk.ABI_VERSION == 11
    assert lib.ykgpu_film_features(None, 2, None, None, None) == 1 and b"null film" in lib.ykgpu_last_error()
    assert lib.ykgpu_film_denoise_guided(None, None, None, None, None, None) == 1 and b"null film" in lib.ykgpu_last_error()
    for name in ("FeatureParams", "GuidedStats", "guided_defaults"):
        assert name in yk.__all__
    assert hasattr(yk.Film, "features") and hasattr(yk.Film, "denoise_guided")


def run_cli(*args):
    return subprocess.run([yk.CLI_PATH, *args], capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("args", [["--denoise-features", "--feature-grid", "5", "a.png"],
                                  ["--denoise-features", "--feature-grid", "0", "a.png"],
                                  ["--aov", "p", "--feature-grid", "x", "a.png"], ["--feature-grid", "2", "a.png"],
                                  ["--denoise", "--feature-grid", "2", "a.png"], ["a.png", "--aov"],
                                  ["--aov", "p", "--feature-grid", "9", "a.png"], ["--denoise-features", "--denoise-k2", "0", "a.png"],
                                  ["--denoise-features", "--denoise-radius", "11", "a.png"]])
def test_cli_reports_bad_feature_options(args):
    r = run_cli(*args)
    assert r.returncode == 2
    assert r.stderr.startswith("raytrace: ") and "see --help" in r.stderr


def test_cli_help_names_the_feature_options():
    out = run_cli("--help").stdout
    for text in ("--denoise-features ", "--feature-grid arg", "--aov arg", ".albedo.png", ".normal.png", ".depth.png",
                 "0.5 * F + 0.5", "F6 / (1 + F6)"):
        assert text in out, text
