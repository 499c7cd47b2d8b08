"""The progressive film's host side (no device): the yardstick itself, the boundary, film files,
the scene hash and the CLI's option handling.

The GPU tests (test_gpu_film.py) compare a film against the oracle's per-sample colours folded in
numpy (film_ref).  Here that fold is shown to be the one-shot render: it reproduces
oracle_lib.render's sums and image byte for byte, in every mode, on tiles and across the seed wrap.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import film_ref
import oracle_lib
import refscenes
import uecraytracing_amd as yk
from uecraytracing_amd import records
from uecraytracing_amd.records import PRECISION_FP32, RNG_XOR128, make_params

CAM = refscenes.reference_camera()
FILM_EXPORTS = ("ykgpu_film_create", "ykgpu_film_destroy", "ykgpu_film_params", "ykgpu_film_accumulate",
                "ykgpu_film_resolve", "ykgpu_film_read", "ykgpu_film_write", "ykgpu_film_error",
                "yk_film_save", "yk_film_load", "yk_scene_hash")

FOLD_CASES = {
    "ref4": (refscenes.ref4, dict(width=16, height=9, spp=13)),
    "wrap": (refscenes.ref4, dict(width=48, height=27, spp=4, seed0=4294967000)),
    "lambert3": (refscenes.lambert3, dict(width=16, height=9, spp=13)),
    "mixed12": (refscenes.mixed12, dict(width=16, height=9, spp=13)),
    "walls2": (refscenes.walls2, dict(width=16, height=9, spp=13)),
    "fp32": (refscenes.ref4, dict(width=16, height=9, spp=13, precision=PRECISION_FP32)),
    "xor128": (refscenes.ref4, dict(width=16, height=9, spp=13, rng=RNG_XOR128)),
    "fp32-xor128": (refscenes.ref4, dict(width=16, height=9, spp=13, precision=PRECISION_FP32, rng=RNG_XOR128)),
    "rows": (refscenes.ref4, dict(width=16, height=9, spp=13, rows=(1, 4, 2))),
    "cols": (refscenes.ref4, dict(width=16, height=9, spp=13, cols=(3, 5, 1))),
}


@pytest.mark.parametrize("case", sorted(FOLD_CASES))
def test_numpy_fold_of_oracle_samples_is_the_one_shot_render(case):
    scene, kw = FOLD_CASES[case]
    p = make_params(max_depth=50, **{"seed0": 404, **kw})
    rgb, sums, _, _ = oracle_lib.render(scene(), CAM, p, want_sums=True)
    S, _ = film_ref.prefixes(film_ref.colours(scene(), CAM, p))
    assert S[-1].tobytes() == sums.tobytes()
    assert film_ref.to_color3b(S[-1], p.samples_per_pixel).tobytes() == rgb.tobytes()


def test_film_entry_points_are_declared_and_exported():
    header = open(os.path.join(os.path.dirname(yk.PKG_DIR), "include", "ykgpu.h")).read()
    lib = yk.load_library()
    for name in FILM_EXPORTS:
        assert name in yk.EXPORTS and hasattr(lib, name) and name + "(" in header, name
    assert "#define YKGPU_ABI_VERSION 11u" in header


def test_film_stats_layout():
    F = records.FilmStats
    assert ctypes.sizeof(F) == 32
    assert (F.pixels.offset, F.pixels_over.offset, F.max_e2.offset, F.samples_done.offset,
            F.samples_target.offset) == (0, 8, 16, 24, 28)


def state(rng, shape):
    """Random doubles of every exponent and sign with the extremes and denormals planted."""
    bits = rng.integers(0, 1 << 64, size=shape, dtype=np.uint64)
    a = bits.view(np.float64).copy()
    a[~np.isfinite(a)] = 1.0
    flat = a.reshape(-1)
    flat[:8] = [0.0, -0.0, 5e-324, -5e-324, 2.2250738585072009e-308, 1.7976931348623157e308,
                -1.7976931348623157e308, 2.2250738585072014e-308]
    return a


def test_film_file_round_trips_exactly(tmp_path):
    rng = np.random.default_rng(7)
    p = make_params(16, 9, 13, rows=(1, 4, 2), cols=(3, 5, 1), seed0=4294967000)
    sums, sumsq = state(rng, (4, 5, 3)), state(rng, (4, 5, 3))
    path = str(tmp_path / "f.ykfilm")
    yk.save_film(path, p, 0xFEDCBA9876543210, 5, sums, sumsq)
    assert os.path.getsize(path) == 32 + ctypes.sizeof(p) + 2 * sums.nbytes
    q, h, done, s2, q2 = yk.load_film(path)
    assert bytes(q) == bytes(p) and h == 0xFEDCBA9876543210 and done == 5
    assert s2.tobytes() == sums.tobytes() and q2.tobytes() == sumsq.tobytes()
    # the header alone, and a capacity too small for the tile
    lib = yk.load_library()
    d = ctypes.c_uint32(0)
    assert lib.yk_film_load(path.encode(), None, None, ctypes.byref(d), None, None, 0) == 0 and d.value == 5
    assert lib.yk_film_load(path.encode(), None, None, None, s2.ctypes.data, q2.ctypes.data, 19) == 1
    # done past the target is not a film state
    with pytest.raises(yk.YkError):
        yk.save_film(path, p, 1, 14, sums, sumsq)


def test_film_load_rejects_truncated_and_foreign_files(tmp_path):
    p = make_params(16, 9, 13)
    z = np.zeros((9, 16, 3))
    good = tmp_path / "good.ykfilm"
    yk.save_film(str(good), p, 1, 3, z, z)
    blob = good.read_bytes()
    yk.load_film(str(good))
    bad = tmp_path / "bad.ykfilm"
    for cut in (0, 7, 31, 32 + 40, len(blob) - 1, len(blob) - 8 * 432):
        bad.write_bytes(blob[:cut])
        with pytest.raises(yk.YkError):
            yk.load_film(str(bad))
    for foreign in (b"yk-scene 1\ncamera 0 0 0\n" + bytes(200), b"\x89PNG\r\n\x1a\n" + blob[8:],
                    blob + b"\0", blob[:8] + b"\x10" + blob[9:]):
        bad.write_bytes(foreign)
        with pytest.raises(yk.YkError):
            yk.load_film(str(bad))
    with pytest.raises(yk.YkError):
        yk.load_film(str(tmp_path / "missing.ykfilm"))


def test_scene_hash_sees_every_field():
    base = yk.scene_hash(refscenes.ref4(), CAM)
    assert base == yk.scene_hash(refscenes.ref4(), CAM)
    seen = {base}

    def changed(edit):
        arr, cam = records.sphere_array(refscenes.ref4()), refscenes.reference_camera()
        edit(arr, cam)
        h = yk.scene_hash(arr, cam)
        assert h not in seen
        seen.add(h)

    for k in range(3):
        changed(lambda a, c, k=k: a[2].center.__setitem__(k, np.nextafter(a[2].center[k], 9.0)))
        changed(lambda a, c, k=k: a[1].albedo.__setitem__(k, 0.25))
    changed(lambda a, c: setattr(a[3], "radius", -0.5))
    changed(lambda a, c: setattr(a[3], "fuzz", 0.125))
    changed(lambda a, c: setattr(a[0], "ior", 1.5))
    changed(lambda a, c: setattr(a[0], "material", records.MATERIAL_DIELECTRIC))
    for name in ("origin", "lower_left_corner", "horizontal", "vertical", "lens_u", "lens_v"):
        changed(lambda a, c, name=name: getattr(c, name).__setitem__(1, 0.375))
    changed(lambda a, c: setattr(c, "lens_radius", 0.05))
    # one sphere fewer, and the same spheres in another tuple order
    assert yk.scene_hash(refscenes.ref4()[:3], CAM) not in seen
    assert yk.scene_hash(refscenes.ref4()[::-1], CAM) not in seen


def run_cli(*args):
    return subprocess.run([yk.CLI_PATH, *args], capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("args", [["--progressive", "0", "a.png"], ["--progressive", "x", "a.png"],
                                  ["--progressive", "-4", "a.png"], ["--until", "x", "a.png"],
                                  ["--until", "-0.5", "a.png"], ["--until", "nan", "a.png"],
                                  ["--stop-after", "0", "a.png"], ["a.png", "--checkpoint", ""],
                                  ["a.png", "--checkpoint"], ["a.png", "--until"]])
def test_cli_reports_bad_film_options(args):
    r = run_cli(*args)
    assert r.returncode == 2
    assert r.stderr.startswith("raytrace: ") and "see --help" in r.stderr


def test_cli_help_names_the_film_options():
    out = run_cli("--help").stdout
    for opt in ("--progressive arg", "--until arg", "--checkpoint arg", "--stop-after arg"):
        assert opt in out


def test_film_without_a_gpu_fails_loudly(tmp_path):
    lib = yk.load_library()
    f = ctypes.c_void_p()
    p = make_params(16, 9, 13)
    assert lib.ykgpu_film_create(None, ctypes.byref(p), ctypes.byref(f)) == records.YK_OK + 1
    assert b"null context" in lib.ykgpu_last_error() and not f.value
    if yk.device_count() > 0:
        pytest.skip("a GPU is visible")
    r = run_cli("--width", "16", "--spp", "13", "--seed0", "404", "--progressive", "4",
                "--checkpoint", str(tmp_path / "c.ykfilm"), str(tmp_path / "o.png"))
    assert r.returncode == 1 and "no HIP device" in r.stderr
    assert not (tmp_path / "o.png").exists() and not (tmp_path / "c.ykfilm").exists()
