"""Pins tests/radiance_ref.py, the restatement the radiance-query GPU tests compare with, to the
reference: its per-path loop must give the reference's own per-sample colours and draw counts
(manifest.json "samples", recorded from the reference's headers), the CPU oracle's colours on a few
hundred samples of three scenes, and the host helper yk_camera_sample_ray must give the restated
start of a camera sample.  No device."""
import subprocess

import numpy as np
import pytest

import cast_ref
import edge_inputs
import golden_data
import oracle_lib
import radiance_ref
import refscenes
import uecraytracing_amd as yk
from uecraytracing_amd import records
from uecraytracing_amd.records import make_params

MAN = golden_data.manifest()
FP64_SAMPLES = sorted(k for k, v in MAN["samples"].items() if v.get("precision", "fp64") == "fp64")
RNGS = {"mt19937": records.RNG_MT19937, "xor128": records.RNG_XOR128}


def spec_case(name):
    spec = MAN["samples"][name]
    sph, cam = golden_data.scene({"scene": spec.get("scene") or name.split("_")[0], **spec})
    p = make_params(spec["W"], spec["H"], spec["spp"], spec["depth"], spec["seed0"], rng=RNGS[spec.get("rng", "mt19937")])
    return spec, list(sph), cam, p


def path_of(sph, cam, p, y, x, s):
    o, d, seed, skip = radiance_ref.camera_start(cam, p, y, x, s)
    return radiance_ref.ray_color(sph, cast_ref.extent(sph), o, d, seed, skip, p.max_depth, p.t_min, p.rng)


def test_the_manifest_has_fp64_samples_of_both_engines():
    rngs = {MAN["samples"][k].get("rng", "mt19937") for k in FP64_SAMPLES}
    assert rngs == {"mt19937", "xor128"}, rngs


@pytest.mark.parametrize("name", FP64_SAMPLES)
def test_restatement_gives_the_reference_samples(name):
    spec, sph, cam, p = spec_case(name)
    for pt in spec["points"]:
        rec = path_of(sph, cam, p, pt["y"], pt["x"], pt["s"])
        assert rec["words"] == pt["draws"], pt
        assert [c.hex() for c in rec["colour"]] == [float.fromhex(v).hex() for v in pt["rgb"]], pt


def oracle_scenes():
    return [("rtiow5",) + tuple(edge_inputs.golden_scene("rtiow5")), ("mixed12", refscenes.mixed12(), refscenes.reference_camera()),
            ("glass48",) + tuple(edge_inputs.golden_scene("glass48"))]


@pytest.mark.parametrize("name,sph,cam", oracle_scenes(), ids=[c[0] for c in oracle_scenes()])
@pytest.mark.parametrize("rng", [records.RNG_MT19937, records.RNG_XOR128], ids=["mt", "x128"])
def test_restatement_equals_the_oracle(name, sph, cam, rng):
    """every 7th pixel of a 16x9x2 image: 42 samples per scene and engine, 250 in all"""
    sph = list(sph)
    p = make_params(16, 9, 2, 50, 404, rng=rng)
    arr = records.sphere_array(sph)
    kinds = set()
    for q in range(0, 16 * 9, 7):
        y, x = divmod(q, 16)
        for s in range(2):
            want, draws = oracle_lib.sample(arr, cam, p, y, x, s)
            rec = path_of(sph, cam, p, y, x, s)
            assert [c.hex() for c in rec["colour"]] == [c.hex() for c in want], (name, y, x, s)
            assert rec["words"] == draws
            kinds.add(rec["flags"] & ~radiance_ref.FALLBACK)
    assert radiance_ref.SKY in kinds and radiance_ref.OOD not in kinds


def start_cases():
    f48, c48 = edge_inputs.golden_scene("final48")  # a thin lens
    return [("pinhole-mt", refscenes.reference_camera(), make_params(32, 18, 6, 50, 404)),
            ("pinhole-x128", refscenes.reference_camera(), make_params(33, 17, 5, 50, 7, rng=records.RNG_XOR128)),
            ("lens-mt", c48, make_params(32, 18, 4, 50, 404)),
            ("lens-x128", c48, make_params(32, 18, 4, 50, 404, rng=records.RNG_XOR128)),
            ("lens-keyed", c48, make_params(32, 18, 4, 50, 404, seed_mode=records.SEED_RANDOM_DEVICE, seed_key=0x1234567890ABCDEF))]


@pytest.mark.parametrize("name,cam,p", start_cases(), ids=[c[0] for c in start_cases()])
def test_camera_sample_ray_equals_the_restated_start(name, cam, p):
    ys, xs, ss = radiance_ref.all_samples(p)
    pick = np.arange(0, len(ys), 5)
    got = yk.camera_sample_rays(cam, p, ys[pick], xs[pick], ss[pick])
    want = radiance_ref.camera_rays(cam, p, ys[pick], xs[pick], ss[pick])
    assert got.tobytes() == want.tobytes()
    assert (got["skip"] >= (8 if cam.lens_radius > 0 else 4)).all() and (got["skip"] % 4 == 0).all()
    if cam.lens_radius > 0:
        assert (got["skip"] > 8).any()  # the rejection loop rejected somewhere


def test_camera_sample_ray_rejects_what_it_cannot_serve():
    cam, lib = refscenes.reference_camera(), yk.load_library()
    out = np.zeros(1, records.PATH_RAY_DTYPE)
    import ctypes
    for p, y, x, s, rc in [(make_params(16, 9, 2), 9, 0, 0, 1), (make_params(16, 9, 2), 0, 16, 0, 1),
                           (make_params(16, 9, 2), 0, 0, 2, 1), (make_params(16, 9, 2, precision=records.PRECISION_FP32), 0, 0, 0, 4),
                           (make_params(16, 9, 2, rng=7), 0, 0, 0, 4)]:
        assert lib.yk_camera_sample_ray(ctypes.byref(cam), ctypes.byref(p), y, x, s, out.ctypes.data) == rc
    assert lib.yk_camera_sample_ray(None, ctypes.byref(make_params(16, 9, 2)), 0, 0, 0, out.ctypes.data) == 1


def test_probe_argument_errors_need_no_device():
    """raytrace --probe: a bad argument is exit status 2 before any device is touched"""
    for args in (["--probe", "3"], ["--probe", "1,1"], ["--probe", "1,1", "--seed0", "4", "--precision", "fp32"],
                 ["--probe", "1,1", "--seed0", "4", "--pick", "1,1"], ["--probe", "400,1", "--seed0", "4"],
                 ["--probe", "1,1", "--seed0", "4", "--spp", "0"]):
        r = subprocess.run([yk.CLI_PATH, *args], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "probe" in r.stderr, (args, r.stderr)
