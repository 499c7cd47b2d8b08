"""Pins tests/gather_ref.py, the restatement the gather-query GPU tests compare with, to the
reference, and the host side of the gather queries to gather_ref.  No device.

The tie (include/ykgpu.h "gather queries"): for a recorded camera sample of the reference
(manifest.json "samples") whose first hit is a lambertian sphere with albedo a, the gather at that
hit's (p, normal) with the sample's (seed, skip), N = 1 and max_depth = D - 1 gives a * sum = the
recorded colour bit for bit, and the path's words = the recorded draws.  Then: yk_gather_sample_rays
against gather_ref's rays as bytes, the records' layout, and the CLI's option errors."""
import ctypes
import subprocess

import numpy as np
import pytest

import gather_ref
import golden_data
import radiance_ref as rr
import uecraytracing_amd as yk
from uecraytracing_amd import records

MT, X128 = records.RNG_MT19937, records.RNG_XOR128


def test_gather_ref_is_tied_to_the_reference_samples():
    cases, total = gather_ref.tie_points()
    compared = 0
    for name, sph, _, p, points, alb, kept in cases:
        recs = gather_ref.path_records(sph, points, 1, p.max_depth - 1, p.t_min, p.rng)
        got = gather_ref.fold(recs)
        for k, pt in enumerate(kept):
            colour = [float(alb[k, c] * got["sum"][k, c]).hex() for c in range(3)]
            assert colour == [float.fromhex(v).hex() for v in pt["rgb"]], (name, pt)
            assert recs["words"][k, 0] == pt["draws"], (name, pt)  # the path's skip is the sample's skip + 6
            assert got["samples"][k] == 1 and not got["flags"][k] & rr.OOD
            compared += 1
    assert total == 264 and compared >= 150, (total, compared)


# ---- the host rays ------------------------------------------------------------------------------

def host_points():
    g = np.random.default_rng(20)
    n = 12
    p = g.uniform(-2.0, 2.0, (n, 3))
    nrm = g.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    nrm[1] *= 3.75  # a non-unit normal
    nrm[2] = -np.abs(nrm[2])  # a negative normal
    nrm[3] = (0.0, -0.0, 0.0)  # a zero normal: no arithmetic, a zero direction
    nrm[4] = (0.0, 0.0, 2.5)
    seeds = g.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    seeds[0] = 0xFFFFFFFE  # wraps within four samples
    return p, nrm, seeds


@pytest.mark.parametrize("rng", [MT, X128], ids=["mt", "x128"])
@pytest.mark.parametrize("skip", [0, 7, 221, 222])
def test_gather_sample_rays_equal_the_restatement(rng, skip):
    p, nrm, seeds = host_points()
    points = gather_ref.make_points(p, nrm, seeds, skip)
    got = yk.gather_sample_rays(points, 4, rng)
    want = gather_ref.sample_rays(points, 4, rng)
    assert got.shape == (len(points), 4) and got.tobytes() == want.tobytes()
    assert (got["seed"][0] == [0xFFFFFFFE, 0xFFFFFFFF, 0, 1]).all() and (got["skip"] == skip + 6).all()
    assert (got["origin"] == p[:, None, :]).all()
    dead = np.zeros(len(points), bool) if skip <= 221 else np.ones(len(points), bool)
    dead[3] = True
    assert not got["direction"][dead].any() and got["direction"][~dead].any(-1).all()
    # one point at a time gives the same records
    lib = yk.load_library()
    one = np.zeros(1, records.PATH_RAY_DTYPE)
    for i in (0, 3, 7):
        for s in range(4):
            assert lib.yk_gather_sample_ray(points[i : i + 1].ctypes.data, rng, s, one.ctypes.data) == 0
            assert one.tobytes() == got[i, s].tobytes()


@pytest.mark.parametrize("rng", [MT, X128], ids=["mt", "x128"])
def test_gather_sample_rays_near_zero_branch(rng):
    """n = -ru exactly: d = n + ru = 0, near_zero, so d = n"""
    seed, skip = 777, 3
    g = rr.Engine(seed, rng, skip)
    ru = g.random_vec()
    ru = rr._divs(ru, rr._sqrt(rr._dot(ru, ru)))
    n = tuple(-c for c in ru)
    points = gather_ref.make_points([(0.5, 0.25, -1.0)] * 2, [n, n], [seed, seed + 1], skip)
    got = yk.gather_sample_rays(points, 1, rng)
    assert got.tobytes() == gather_ref.sample_rays(points, 1, rng).tobytes()
    assert tuple(got["direction"][0, 0]) == n  # the branch
    assert tuple(got["direction"][1, 0]) != n  # another seed: the sum


def test_gather_sample_rays_arguments():
    lib = yk.load_library()
    pt, out = np.zeros(1, records.GATHER_POINT_DTYPE), np.zeros(1, records.PATH_RAY_DTYPE)
    assert lib.yk_gather_sample_ray(None, MT, 0, out.ctypes.data) == 1
    assert lib.yk_gather_sample_ray(pt.ctypes.data, MT, 0, None) == 1
    assert lib.yk_gather_sample_ray(pt.ctypes.data, 2, 0, out.ctypes.data) == 4
    assert lib.yk_gather_sample_rays(None, 1, MT, 1, out.ctypes.data) == 1
    assert lib.yk_gather_sample_rays(pt.ctypes.data, 1, 2, 1, out.ctypes.data) == 4
    assert lib.yk_gather_sample_rays(None, 0, MT, 1, None) == 0
    assert yk.gather_sample_rays(pt[:0], 3).shape == (0, 3)
    with pytest.raises(yk.YkError):
        yk.gather_sample_rays(pt, 0)
    with pytest.raises(yk.YkError):
        yk.gather_points(np.zeros((2, 3)), np.zeros((3, 3)), 1)


# ---- records and the CLI ------------------------------------------------------------------------

def test_record_sizes_and_offsets():
    P, G, A, S = records.GatherPoint, records.Gather, records.GatherParams, records.GatherStats
    assert [ctypes.sizeof(c) for c in (P, G, A, S)] == [64, 64, 32, 64]
    assert (P.p.offset, P.n.offset, P.seed.offset, P.skip.offset, P.reserved.offset) == (0, 24, 48, 52, 56)
    assert (G.sum.offset, G.sumsq.offset, G.samples.offset, G.open.offset, G.flags.offset, G.reserved.offset) == (0, 24, 48, 52, 56, 60)
    assert (A.n_samples.offset, A.max_depth.offset, A.rng.offset, A.flags.offset, A.t_min.offset, A.reserved.offset) == (0, 4, 8, 12, 16, 24)
    assert (S.kernel_ms.offset, S.total_ms.offset, S.starts_ms.offset, S.fold_ms.offset, S.points.offset, S.rays.offset,
            S.open.offset, S.out_of_domain.offset, S.mt_fallbacks.offset) == (0, 8, 16, 24, 32, 40, 48, 56, 60)
    for dt, cls in ((records.GATHER_POINT_DTYPE, P), (records.GATHER_DTYPE, G)):
        assert dt.itemsize == ctypes.sizeof(cls)
        for name, _ in cls._fields_:
            assert dt.fields[name][1] == getattr(cls, name).offset, name
    header = open(golden_data.GOLDEN + "/../../include/ykgpu.h").read()
    for name in ("yk_gather_point", "yk_gather", "yk_gather_params", "yk_gather_stats"):
        assert "typedef struct %s {" % name in header


def test_gather_argument_errors_need_no_device():
    """raytrace --gather: a bad argument is exit status 2 before any device is touched"""
    for args in (["--gather", "3"], ["--gather", "1,1"], ["--gather", "1,1", "--seed0", "4", "--precision", "fp32"],
                 ["--gather", "1,1", "--seed0", "4", "--pick", "1,1"], ["--gather", "1,1", "--seed0", "4", "--probe", "1,1"],
                 ["--gather", "400,1", "--seed0", "4"], ["--gather", "1,225", "--seed0", "4"],
                 ["--gather", "1,1", "--seed0", "4", "--spp", "0"], ["--gather", "x,1", "--seed0", "4"]):
        r = subprocess.run([yk.CLI_PATH, *args], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "gather" in r.stderr and "see --help" in r.stderr, (args, r.stderr)
    r = subprocess.run([yk.CLI_PATH, "--help"], capture_output=True, text=True, timeout=60)
    assert "--gather arg" in r.stdout
