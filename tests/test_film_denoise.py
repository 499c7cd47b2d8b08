"""The film denoise filter's host side (no device): the numpy yardstick (film_denoise_ref) against
the definition of include/ykgpu.h "film denoise", and the new records and entry points.

The GPU tests (test_gpu_film_denoise.py) compare ykgpu_film_denoise with the yardstick byte for
byte.  Here the yardstick is pinned to the specification: its identities (radius 0 is the mean),
its range (a weighted mean with non-negative weights stays inside the input's range), and the
mean squared errors against a 1024-spp image that the definition gives on the oracle's samples
(figures from the feature's specification, reproduced to 1e-9 relative — not from the code under
test)."""
import ctypes
import os

import numpy as np
import pytest

import film_adaptive_ref as far
import film_denoise_ref as fdr
import film_ref
import refscenes
import uecraytracing_amd as yk
from uecraytracing_amd import records
from uecraytracing_amd.records import make_params

CAM = refscenes.reference_camera()

# scene, width, height, samples, raw MSE, filtered MSE (None: only the ratio is specified), ratio
MSE_CASES = {
    "ref4": (refscenes.ref4, 48, 27, 8, 0.0014187406884441007, 0.0005264189871792214, 0.371),
    "lambert3": (refscenes.lambert3, 48, 27, 8, None, None, 0.292),
    "mixed12": (refscenes.mixed12, 64, 36, 16, 0.0007955148701554881, 0.0003978491064184538, 0.500),
}


def state(scene, width, height, n):
    S, Q = film_ref.prefixes(film_ref.colours(scene(), CAM, make_params(width, height, n, 50, 404)))
    return S, Q


@pytest.mark.parametrize("patch", [0, 3])
def test_radius_zero_returns_the_mean_byte_for_byte(patch):
    S, Q = state(refscenes.ref4, 16, 9, 4)
    out = fdr.denoise(S[4], Q[4], 4, radius=0, patch=patch)
    assert out.tobytes() == (S[4] / 4.0).tobytes()


def check_finite_and_in_range(out, m):
    assert np.isfinite(out).all()
    for c in range(3):
        assert m[:, :, c].min() <= out[:, :, c].min() and out[:, :, c].max() <= m[:, :, c].max(), c


def test_window_and_patch_larger_than_the_image():
    S, Q = state(refscenes.ref4, 16, 9, 4)
    m, _ = fdr.moments(S[4], Q[4], 4)
    out = fdr.denoise(S[4], Q[4], 4, radius=10, patch=3)
    check_finite_and_in_range(out, m)
    assert out.tobytes() != m.tobytes()  # (it filtered)


def test_non_uniform_state():
    S, Q = state(refscenes.ref4, 16, 9, 20)
    e2 = film_ref.e2_map(S[4], Q[4], 4)
    counts = np.where(e2 > np.median(e2), 20, 4).astype(np.uint32)
    assert 0 < int((counts == 20).sum()) < counts.size
    sums, sumsq = far.at_counts(S, counts), far.at_counts(Q, counts)
    m, _ = fdr.moments(sums, sumsq, counts)
    assert m.tobytes() == np.where((counts == 20)[:, :, None], S[20] / 20.0, S[4] / 4.0).tobytes()
    check_finite_and_in_range(fdr.denoise(sums, sumsq, counts), m)


@pytest.mark.parametrize("case", sorted(MSE_CASES))
def test_it_denoises(case):
    scene, w, h, n, raw_spec, filt_spec, ratio_spec = MSE_CASES[case]
    truth = fdr.truth(scene(), CAM, w, h)
    S, Q = state(scene, w, h, n)
    raw, filt = fdr.mse(S[n] / float(n), truth), fdr.mse(fdr.denoise(S[n], Q[n], n), truth)
    print(case, "raw", repr(raw), "filtered", repr(filt), "ratio", filt / raw)
    assert filt <= 0.8 * raw
    # the yardstick is the specification's filter: its figures, to 1e-9 relative
    if raw_spec is not None:
        assert abs(raw - raw_spec) <= 1e-9 * raw_spec and abs(filt - filt_spec) <= 1e-9 * filt_spec
    assert abs(filt / raw - ratio_spec) <= 0.0005  # (the specification's ratio, given to three decimals)


def test_records_and_defaults():
    P, S = records.DenoiseParams, records.DenoiseStats
    assert ctypes.sizeof(P) == 32 and ctypes.sizeof(S) == 24
    assert (P.radius.offset, P.patch.offset, P.k2.offset, P.alpha.offset, P.eps.offset) == (0, 4, 8, 16, 24)
    assert (S.moments_ms.offset, S.filter_ms.offset, S.total_ms.offset) == (0, 8, 16)
    assert yk.denoise_defaults().as_dict() == dict(radius=5, patch=1, k2=0.5, alpha=1.0, eps=1e-10) == fdr.DEFAULTS
    lib = yk.load_library()
    assert lib.yk_denoise_defaults(None) == 1
    assert lib.ykgpu_abi_version() == yk.ABI_VERSION == 11


def test_entry_points_are_declared_and_exported():
    header = open(os.path.join(os.path.dirname(yk.PKG_DIR), "include", "ykgpu.h")).read()
    lib = yk.load_library()
    for name in ("yk_denoise_defaults", "ykgpu_film_denoise"):
        assert name in yk.EXPORTS and hasattr(lib, name) and name + "(" in header, name
    assert "typedef struct yk_denoise_params {" in header and "typedef struct yk_denoise_stats {" in header
    assert "#define YKGPU_ABI_VERSION 11u" in header
    assert lib.ykgpu_film_denoise(None, None, None, None, None) == 1 and b"null film" in lib.ykgpu_last_error()


def run_cli(*args):
    import subprocess
    return subprocess.run([yk.CLI_PATH, *args], capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("args", [["--denoise", "--denoise-radius", "11", "a.png"], ["--denoise", "--denoise-patch", "4", "a.png"],
                                  ["--denoise", "--denoise-k2", "0", "a.png"], ["--denoise", "--denoise-k2", "nan", "a.png"],
                                  ["--denoise", "--denoise-radius", "x", "a.png"], ["--denoise-radius", "3", "a.png"],
                                  ["a.png", "--denoise", "--denoise-k2"]])
def test_cli_reports_bad_denoise_options(args):
    r = run_cli(*args)
    assert r.returncode == 2
    assert r.stderr.startswith("raytrace: ") and "see --help" in r.stderr


def test_cli_help_names_the_denoise_options():
    out = run_cli("--help").stdout
    for opt in ("--denoise ", "--denoise-radius arg", "--denoise-patch arg", "--denoise-k2 arg"):
        assert opt in out
