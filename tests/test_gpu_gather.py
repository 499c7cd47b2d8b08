"""ykgpu_gather_points on the MI355X (include/ykgpu.h "gather queries"): every record compared byte
for byte, with no tolerance, with the composed route the gather replaces (yk_gather_sample_rays on
the host, ykgpu_radiance_rays, the numpy fold), with the Python restatement of the definition
(gather_ref, pinned to the reference by tests/test_gather_ref.py) and, through the tie to the render,
with the reference's own recorded per-sample colours (manifest.json "samples").

The inputs are the smallest that take every path of the two kernels and the chunk loop: sample
counts below, at and above the starts kernel's four slots per lane, point counts around a wave and a
block and past the resident lanes, a call one chunk and three points long, one point at the largest
sample count, paths past mt19937's lazy words, the skip limit from both sides, points that are not
points, the error codes, device memory on torch's stream, a film, a second scene and the CLI."""
import ctypes
import subprocess

import numpy as np
import pytest

import cast_ref
import edge_inputs
import gather_ref
import radiance_ref as rr
import refscenes
import uecraytracing_amd as yk
from uecraytracing_amd import records
from uecraytracing_amd.records import make_params

pytestmark = pytest.mark.gpu

CAM = refscenes.reference_camera()
MT, X128 = records.RNG_MT19937, records.RNG_XOR128
INF, NAN = float("inf"), float("nan")
YK_ERR_INVALID, YK_ERR_UNSUPPORTED, YK_ERR_NO_SCENE = 1, 4, 5
CHUNK_RAYS = 1 << 22  # yk_host_internal.hpp kRadChunk: a chunk holds max(1, CHUNK_RAYS // N) points


@pytest.fixture(scope="module")
def ren():
    r = yk.Renderer(0)
    yield r
    r.close()


def same(got, want, what=""):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    bad = int((got.view(np.uint64).reshape(-1, 8) != want.view(np.uint64).reshape(-1, 8)).any(1).sum())
    assert got.tobytes() == want.tobytes(), f"{what}: {bad} of {len(want)} records differ"


def grid_points(ren, cam, W=16, H=9, seed0=5000, skip=0):
    """GATHER_POINT_DTYPE[K]: the first hits of the W x H pixel-centre rays, as cast_rays returns them
    (the scene is set), with seeds of their own"""
    o, d = cast_ref.pixel_rays(cam, W, H)
    hits = ren.cast_rays(o, d)
    hits = hits[(hits["flags"] & records.HIT_HIT) != 0]
    seeds = (seed0 + 7919 * np.arange(len(hits), dtype=np.uint64)) % 2 ** 32
    return gather_ref.make_points(hits["p"], hits["normal"], seeds.astype(np.uint32), skip)


def composed(ren, points, n, max_depth=50, t_min=records.T_MIN, rng=MT, **kw):
    """the route the gather replaces: the path rays on the host, the radiance query, the numpy fold"""
    rays = yk.gather_sample_rays(points, n, rng)
    recs = ren.radiance_rays(rays.reshape(-1), max_depth, t_min, rng, **kw).reshape(rays.shape)
    return gather_ref.fold(recs), recs


# ---- 1. a gather is the fold of its radiance queries ----------------------------------------------

def fold_scenes():
    return [("ref4-mt", refscenes.ref4(), CAM, MT), ("ref4-x128", refscenes.ref4(), CAM, X128),
            ("final48-lens",) + tuple(edge_inputs.golden_scene("final48")) + (MT,)]


@pytest.mark.parametrize("n", [1, 3, 4, 5, 64])
@pytest.mark.parametrize("name,sph,cam,rng", fold_scenes(), ids=[c[0] for c in fold_scenes()])
def test_gather_is_the_fold_of_its_queries(ren, name, sph, cam, rng, n):
    sph = list(sph)
    ren.set_scene(sph, cam)
    points = grid_points(ren, cam)
    assert len(points) >= 60
    got = ren.gather_points(points, n, 50, records.T_MIN, rng)
    want, recs = composed(ren, points, n, rng=rng)
    same(got, want, f"{name} N {n}")
    assert (got["samples"] == n).all() and not got["reserved"].any() and not (got["flags"] & rr.OOD).any()
    assert got["open"].sum() > 0 and (got["sum"] >= 0).all() and got["sum"].any(1).sum() > len(points) // 2
    st = ren.gather_stats()
    assert (st["points"], st["rays"], st["open"]) == (len(points), len(points) * n, int(got["open"].sum()))
    assert st["out_of_domain"] == 0 and st["kernel_ms"] > 0 and st["total_ms"] >= st["kernel_ms"] > st["fold_ms"] > 0
    pick = np.linspace(0, len(points) - 1, 6).astype(int)
    same(got[pick], gather_ref.gather(sph, points[pick], n, 50, records.T_MIN, rng), f"{name} N {n} against gather_ref")


# ---- 2. the tie to the render, on the reference's recorded samples --------------------------------

def test_the_tie_to_the_reference_samples(ren):
    cases, total = gather_ref.tie_points()
    compared = 0
    for name, sph, cam, p, points, alb, kept in cases:
        ren.set_scene(sph, cam)
        rays = yk.camera_sample_rays(cam, p, [q["y"] for q in kept], [q["x"] for q in kept], [q["s"] for q in kept])
        hits = ren.cast_rays(rays["origin"], rays["direction"], p.t_min)
        here = gather_ref.make_points(hits["p"], hits["normal"], rays["seed"], rays["skip"])
        assert here.tobytes() == points.tobytes(), name
        got = ren.gather_points(here, 1, p.max_depth - 1, p.t_min, p.rng)
        _, recs = composed(ren, here, 1, p.max_depth - 1, p.t_min, p.rng)
        for k, pt in enumerate(kept):
            colour = [float(alb[k, c] * got["sum"][k, c]).hex() for c in range(3)]
            assert colour == [float.fromhex(v).hex() for v in pt["rgb"]], (name, pt)
            # skip + 6 + the path's own words: the record's words count its skip
            assert recs["words"][k, 0] == pt["draws"] and recs["words"][k, 0] >= here["skip"][k] + 6, (name, pt)
            assert bool(got["flags"][k] & rr.FALLBACK) == (p.rng == MT and pt["draws"] > rr.LAZY_WORDS)
            compared += 1
    assert total == 264 and compared >= 150, (total, compared)


# ---- 3. deep paths --------------------------------------------------------------------------------

def test_deep_paths_reach_the_points_flags(ren):
    sph, p = refscenes.walls2(), edge_inputs.deep_params(edge_inputs.FP64, MT)
    ren.set_scene(sph, CAM)
    points = grid_points(ren, CAM)
    got = ren.gather_points(points, 4, p.max_depth, p.t_min, MT)
    want, recs = composed(ren, points, 4, p.max_depth, p.t_min, MT)
    same(got, want, "deep")
    fb = ((recs["flags"] & rr.FALLBACK) != 0).any(1)
    assert fb.sum() >= 3 and recs["words"].max() > 1248 and recs["segments"].max() > 200
    assert (((got["flags"] & rr.FALLBACK) != 0) == fb).all()
    assert ren.gather_stats()["mt_fallbacks"] == int(fb.sum())
    x = ren.gather_points(points, 4, p.max_depth, p.t_min, X128)
    same(x, composed(ren, points, 4, p.max_depth, p.t_min, X128)[0], "deep xor128")
    assert not (x["flags"] & rr.FALLBACK).any()


# ---- 4. batch shapes ------------------------------------------------------------------------------

def test_batch_shapes_and_refill(ren):
    sph, cam = edge_inputs.golden_scene("final48")
    ren.set_scene(sph, cam)
    base = grid_points(ren, cam, 32, 18)
    assert len(base) >= 257
    full = ren.gather_points(base[:257], 3)
    same(full, composed(ren, base[:257], 3)[0], "257 points")
    for n in (1, 63, 64, 65, 255, 257):
        same(ren.gather_points(base[:n], 3), full[:n], f"batch of {n}")
        assert ren.gather_stats()["points"] == n
    lanes = ren.radiance_stats()["lanes"]
    assert lanes >= 256 and lanes % 256 == 0
    reps = lanes // len(base) + 2
    many = np.tile(base, reps)
    many["seed"] = (many["seed"].astype(np.uint64) + 104729 * np.arange(len(many), dtype=np.uint64)) % 2 ** 32
    assert len(many) > lanes  # lanes refill
    got = ren.gather_points(many, 1)
    same(got, composed(ren, many, 1)[0], "past the resident lanes")
    # a record depends on its point alone: a permuted batch gives the permuted records
    perm = np.random.default_rng(3).permutation(4096)
    same(ren.gather_points(many[:4096][perm], 3), ren.gather_points(many[:4096], 3)[perm], "permutation")


# ---- 5. the chunk seam ----------------------------------------------------------------------------

def test_the_chunk_seam(ren):
    """a call one chunk and three points long: a second round of launches, no fold across the seam"""
    sph, cam = edge_inputs.golden_scene("rtiow5")
    ren.set_scene(sph, cam)
    base = grid_points(ren, cam)[:64]
    assert len(base) == 64
    want = ren.gather_points(base, 5)
    same(want, composed(ren, base, 5)[0], "the base points")
    n = CHUNK_RAYS // 5 + 3
    reps = n // 64 + 1
    got = ren.gather_points(np.tile(base, reps)[:n], 5)
    assert len(got) == n and got.tobytes() == np.tile(want, reps)[:n].tobytes()
    st = ren.gather_stats()
    assert st["points"] == n and st["rays"] == 5 * n


# ---- 6. one point at the largest sample count -----------------------------------------------------

def test_one_point_at_65536_samples(ren):
    """cp = 64 points a chunk, one of them used; xor128, against the composed route"""
    ren.set_scene(refscenes.ref4(), CAM)
    point = grid_points(ren, CAM)[40:41]
    point["seed"] = 0xFFFF8000  # the seeds wrap half-way
    got = ren.gather_points(point, 65536, 50, records.T_MIN, X128)
    same(got, composed(ren, point, 65536, rng=X128)[0], "N 65536")
    assert got["samples"][0] == 65536 and 0 < got["open"][0] < 65536


# ---- 7. guards, arguments, plumbing ---------------------------------------------------------------

def test_linear_scan_gives_the_same_bytes(ren):
    sph, cam = edge_inputs.golden_scene("final48")
    ren.set_scene(sph, cam)
    points = grid_points(ren, cam)
    same(ren.gather_points(points, 4, linear_scan=True, count_work=True), ren.gather_points(points, 4), "linear scan")


def test_the_skip_limit(ren):
    sph = refscenes.mixed12()
    ren.set_scene(sph, CAM)
    for rng in (MT, X128):
        for skip in (7, 221):
            points = grid_points(ren, CAM, skip=skip)
            got = ren.gather_points(points, 3, 50, records.T_MIN, rng)
            want, recs = composed(ren, points, 3, rng=rng)
            same(got, want, f"skip {skip}")
            assert not (got["flags"] & rr.OOD).any() and (recs["words"] >= skip + 6).all()
            same(got[:4], gather_ref.gather(sph, points[:4], 3, 50, records.T_MIN, rng), f"skip {skip} against gather_ref")
        points = grid_points(ren, CAM, skip=221)
        points["skip"][::3] = 222
        points["skip"][1] = 0xFFFFFFFF
        over = points["skip"] > 221
        got = ren.gather_points(points, 3, 50, records.T_MIN, rng)
        same(got, composed(ren, points, 3, rng=rng)[0], "skip 222 among 221")
        dead = np.zeros(int(over.sum()), records.GATHER_DTYPE)
        dead["samples"], dead["flags"] = 3, rr.OOD
        assert got[over].tobytes() == dead.tobytes() and not (got["flags"][~over] & rr.OOD).any()
        assert ren.gather_stats()["out_of_domain"] == int(over.sum())


def test_points_outside_the_domain_do_not_void_a_batch(ren):
    sph = refscenes.mixed12()
    ren.set_scene(sph, CAM)
    clean = grid_points(ren, CAM)
    points = clean.copy()
    assert len(points) >= 60
    bad = {3: ("p", (NAN, 0.0, -1.0)), 9: ("p", (0.0, INF, 0.0)), 17: ("n", (0.0, 0.0, 0.0)), 18: ("n", (-0.0, 0.0, -0.0)),
           33: ("n", (NAN, 0.0, 1.0)), 40: ("n", (0.0, -INF, 0.0)), 41: ("p", (2.0 ** 501, 0.0, 0.0)), 59: ("n", (INF, INF, INF))}
    for i, (which, v) in bad.items():
        points[which][i] = v
    good = np.setdiff1d(np.arange(len(points)), list(bad))
    for rng in (MT, X128):
        got = ren.gather_points(points, 5, 50, records.T_MIN, rng)
        st = ren.gather_stats()
        assert st["out_of_domain"] == len(bad) and st["points"] == len(points)
        same(got, composed(ren, points, 5, rng=rng)[0], "mixed batch")
        dead = np.zeros(1, records.GATHER_DTYPE)
        dead["samples"], dead["flags"] = 5, rr.OOD
        for i in bad:
            assert got[i : i + 1].tobytes() == dead.tobytes(), i
        same(got[good], ren.gather_points(clean, 5, 50, records.T_MIN, rng)[good], "the other points")
    same(got[[3, 17, 33]], gather_ref.gather(sph, points[[3, 17, 33]], 5, 50, records.T_MIN, X128), "against gather_ref")


def test_error_codes(ren):
    lib = yk.load_library()
    pt, rec = np.zeros(1, records.GATHER_POINT_DTYPE), np.zeros(1, records.GATHER_DTYPE)
    pt["p"], pt["n"] = (0.0, 0.0, -0.5), (0.0, 0.0, 1.0)

    def par(n=4, max_depth=50, rng=MT, flags=0, t_min=0.001, reserved=0):
        return ctypes.byref(records.GatherParams(n, max_depth, rng, flags, t_min, reserved))

    r, o = pt.ctypes.data, rec.ctypes.data
    with yk.Renderer(0) as fresh:
        assert lib.ykgpu_gather_points(fresh._ctx, par(), r, 1, o) == YK_ERR_NO_SCENE
        assert lib.ykgpu_gather_points_async(fresh._ctx, par(), 16, 1, 16, None) == YK_ERR_NO_SCENE
        assert lib.ykgpu_gather_points(fresh._ctx, par(), None, 0, None) == 0
        with pytest.raises(yk.YkError):
            fresh.gather([(0.0, 0.0, -0.5)], [(0.0, 0.0, 1.0)], 1, 4)
    ren.set_scene(refscenes.ref4(), CAM)
    ctx = ren._ctx
    assert lib.ykgpu_gather_points(ctx, par(), r, 1, o) == 0 and rec["samples"][0] == 4
    assert lib.ykgpu_gather_points(ctx, par(), None, 0, None) == 0
    assert lib.ykgpu_gather_points_async(ctx, par(), None, 0, None, None) == 0
    assert lib.ykgpu_gather_points(None, par(), r, 1, o) == YK_ERR_INVALID
    assert lib.ykgpu_gather_points(ctx, None, r, 1, o) == YK_ERR_INVALID
    assert lib.ykgpu_gather_points(ctx, par(), None, 1, o) == YK_ERR_INVALID
    assert lib.ykgpu_gather_points(ctx, par(), r, 1, None) == YK_ERR_INVALID
    assert lib.ykgpu_gather_points(ctx, par(flags=4), r, 1, o) == YK_ERR_INVALID
    assert b"flag" in lib.ykgpu_last_error()
    for n in (0, 65537):
        assert lib.ykgpu_gather_points(ctx, par(n=n), r, 1, o) == YK_ERR_INVALID
        assert b"n_samples" in lib.ykgpu_last_error()
    for depth in (0, 65536):
        assert lib.ykgpu_gather_points(ctx, par(max_depth=depth), r, 1, o) == YK_ERR_INVALID
    assert lib.ykgpu_gather_points(ctx, par(max_depth=65535), r, 1, o) == 0
    for t in (-0.001, INF, NAN):
        assert lib.ykgpu_gather_points(ctx, par(t_min=t), r, 1, o) == YK_ERR_INVALID
    assert lib.ykgpu_gather_points(ctx, par(t_min=0.0), r, 1, o) == 0
    assert lib.ykgpu_gather_points(ctx, par(reserved=1), r, 1, o) == YK_ERR_INVALID
    assert lib.ykgpu_gather_points(ctx, par(rng=2), r, 1, o) == YK_ERR_UNSUPPORTED
    assert lib.ykgpu_gather_points_async(ctx, par(), None, 1, None, None) == YK_ERR_INVALID
    assert lib.ykgpu_gather_points_async(ctx, par(), 8, 1, 16, None) == YK_ERR_INVALID  # (not 16-byte aligned)
    assert lib.ykgpu_gather_get_stats(ctx, None) == YK_ERR_INVALID
    with pytest.raises(yk.YkError):
        ren.gather(np.zeros((2, 3)), np.zeros((3, 3)), 1, 4)


def test_device_tensors_on_torchs_stream(ren):
    torch = pytest.importorskip("torch")
    sph, cam = edge_inputs.golden_scene("final48")
    ren.set_scene(sph, cam)
    points = grid_points(ren, cam)
    n = len(points)
    side = torch.cuda.Stream()
    for rng in (MT, X128):
        host = ren.gather_points(points, 5, 50, records.T_MIN, rng)
        with torch.cuda.stream(side):  # torch's current stream: the tensors are made and gathered on it
            t_pts = torch.from_numpy(points.view(np.float64).reshape(n, 8)).cuda()
            t_out = torch.full((n, 8), -7.25, dtype=torch.float64, device="cuda")
            stream = torch.cuda.current_stream()
            assert stream.cuda_stream == side.cuda_stream != 0
            ren.gather_device(t_pts.data_ptr(), n, t_out.data_ptr(), 5, 50, records.T_MIN, rng, stream_ptr=stream.cuda_stream)
            stream.synchronize()
        assert t_out.cpu().numpy().tobytes() == host.tobytes()
    assert ren.gather_stats()["points"] == n  # (the asynchronous gathers record nothing)
    # a radiance query after an asynchronous gather waits for it: they share staging and scratch
    rays = yk.gather_sample_rays(points, 5, MT).reshape(-1)
    want = ren.radiance_rays(rays)
    with torch.cuda.stream(side):
        ren.gather_device(t_pts.data_ptr(), n, t_out.data_ptr(), 5, stream_ptr=side.cuda_stream)
    same(ren.radiance_rays(rays), want, "a query behind a gather")
    side.synchronize()
    assert t_out.cpu().numpy().tobytes() == ren.gather_points(points, 5).tobytes()


def test_a_gather_between_two_film_chunks_leaves_the_film_alone(ren):
    sph = refscenes.mixed12()
    ren.set_scene(sph, CAM)
    p = make_params(32, 18, 8, 50, 404)
    want = ren.render_sums(p)
    points = grid_points(ren, CAM)
    alone = ren.gather_points(points, 4)
    with ren.film(p) as film:
        film.accumulate(3)
        got = ren.gather_points(points, 4)
        film.accumulate(5)
        sums, _, done = film.read()
    assert done == 8 and sums.tobytes() == want.tobytes()
    same(got, alone, "beside a film")


def test_a_gather_after_a_second_set_scene_answers_for_the_new_scene(ren):
    ren.set_scene(refscenes.ref4(), CAM)
    points = grid_points(ren, CAM)
    first = ren.gather_points(points, 4)
    ren.set_scene(refscenes.mixed12(), CAM)
    second = ren.gather_points(points, 4)
    same(second, composed(ren, points, 4)[0], "the new scene")
    assert first.tobytes() != second.tobytes()
    ren.set_scene(refscenes.ref4(), CAM)
    same(ren.gather_points(points, 4), first, "back to the first scene")
    assert ren.stats()["device_bytes"] >= len(points) * 128  # the staging is counted


def test_cli_gather_equals_the_renderer(ren):
    W, H, N, depth, seed0 = 64, 36, 8, 20, 404
    ren.set_scene(refscenes.ref4(), CAM)
    o, d = cast_ref.pixel_rays(CAM, W, H)
    hits = ren.cast_rays(o, d)
    for x, y in ((20, 18), (40, 30), (0, 0)):
        r = subprocess.run([yk.CLI_PATH, "--width", str(W), "--spp", str(N), "--depth", str(depth), "--seed0", str(seed0),
                            "--gather", f"{x},{y}"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        hit = hits[y * W + x]
        if not hit["flags"] & records.HIT_HIT:
            assert r.stdout == f"gather {x} {y}: miss\n"
            assert (x, y) == (0, 0)
            continue
        g = ren.gather([hit["p"]], [hit["normal"]], seed0, N, 0, depth)[0]
        s, m = g["sum"], [float(c) / N for c in g["sum"]]
        line = ("gather %d %d: id %d samples %d sum (%.17g, %.17g, %.17g) mean (%.17g, %.17g, %.17g) open %d\n"
                % (x, y, hit["id"], N, s[0], s[1], s[2], m[0], m[1], m[2], g["open"]))
        assert r.stdout == line
