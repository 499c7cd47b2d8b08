"""ykgpu_radiance_rays on the MI355X (include/ykgpu.h "radiance queries"): every record compared byte
for byte, with no tolerance, with the reference's own per-sample results (manifest.json "samples"),
the golden per-pixel sums, the CPU oracle and the Python restatement of the definition
(radiance_ref, pinned to the reference by tests/test_radiance_ref.py).

The inputs are the smallest that take every path of the two kernels: the reference's recorded
samples, whole small images through the query against the render, paths hundreds of segments deep
(the scratch engine and the spilled attenuation ids), discards across the lazy cursors' end and a
twist, rays that start on surfaces and inside glass, every way a path ends, batch sizes around a
wave and a block and past the resident lanes (so lanes refill), the scan guards, rays outside the
domain, the error codes, device memory on torch's stream, a film and a second scene."""
import ctypes

import numpy as np
import pytest

import cast_ref
import edge_inputs
import golden_data
import oracle_lib
import radiance_ref as rr
import refscenes
import uecraytracing_amd as yk
from uecraytracing_amd import records
from uecraytracing_amd.records import lambertian, make_params, metal

pytestmark = pytest.mark.gpu

CAM = refscenes.reference_camera()
MT, X128 = records.RNG_MT19937, records.RNG_XOR128
MAN = golden_data.manifest()
FP64_SAMPLES = sorted(k for k, v in MAN["samples"].items() if v.get("precision", "fp64") == "fp64")
RNGS = {"mt19937": MT, "xor128": X128}
INF, NAN = float("inf"), float("nan")
YK_ERR_INVALID, YK_ERR_UNSUPPORTED, YK_ERR_NO_SCENE = 1, 4, 5
ENDS = rr.SKY | rr.ABSORBED | rr.DEPTH | rr.OOD


@pytest.fixture(scope="module")
def ren():
    r = yk.Renderer(0)
    yield r
    r.close()


def same(got, want, what=""):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    bad = int((got.view(np.uint64).reshape(-1, 8) != want.view(np.uint64).reshape(-1, 8)).any(1).sum())
    assert got.tobytes() == want.tobytes(), f"{what}: {bad} of {len(want)} records differ"


def query(ren, rays, p, **kw):
    return ren.radiance_rays(rays, p.max_depth, p.t_min, p.rng, **kw)


def all_rays(cam, p):
    return yk.camera_sample_rays(cam, p, *rr.all_samples(p))


def oracle_samples(sph, cam, p, ys, xs, ss):
    arr = records.sphere_array(list(sph))
    res = [oracle_lib.sample(arr, cam, p, int(y), int(x), int(s)) for y, x, s in zip(ys, xs, ss)]
    return np.array([r[0] for r in res], np.float64), np.array([r[1] for r in res], np.uint64)


# ---- 1. the reference's recorded samples ----------------------------------------------------------

@pytest.mark.parametrize("name", FP64_SAMPLES)
def test_reference_points(ren, name):
    spec = MAN["samples"][name]
    sph, cam = golden_data.scene({"scene": spec.get("scene") or name.split("_")[0], **spec})
    sph = list(sph)
    p = make_params(spec["W"], spec["H"], spec["spp"], spec["depth"], spec["seed0"], rng=RNGS[spec.get("rng", "mt19937")])
    ren.set_scene(sph, cam)
    for pt in spec["points"]:  # one ray per query
        ray = yk.camera_sample_rays(cam, p, [pt["y"]], [pt["x"]], [pt["s"]])
        rec = query(ren, ray, p)[0]
        assert [float(c).hex() for c in rec["colour"]] == [float.fromhex(v).hex() for v in pt["rgb"]], pt
        assert rec["words"] == pt["draws"], pt
        assert bool(rec["flags"] & rr.FALLBACK) == (p.rng == MT and pt["draws"] > rr.LAZY_WORDS)
    pts = spec["points"][:6]
    rays = yk.camera_sample_rays(cam, p, [q["y"] for q in pts], [q["x"] for q in pts], [q["s"] for q in pts])
    same(query(ren, rays, p), rr.radiance(sph, rays, p.max_depth, p.t_min, p.rng), name)


# ---- 2. the query equals the render ---------------------------------------------------------------

def render_cases():
    return [("ref4", refscenes.ref4(), CAM, make_params(32, 18, 6, 50, 404), "ref4_32x18x6_d50_s404"),
            ("ref4-x128", refscenes.ref4(), CAM, make_params(32, 18, 6, 50, 404, rng=X128), "ref4_32x18x6_d50_s404_x128"),
            ("final48-lens",) + tuple(edge_inputs.golden_scene("final48")) + (make_params(32, 18, 4, 50, 404), None)]


@pytest.mark.parametrize("name,sph,cam,p,golden", render_cases(), ids=[c[0] for c in render_cases()])
def test_query_equals_the_render(ren, name, sph, cam, p, golden):
    ren.set_scene(sph, cam)
    rays = all_rays(cam, p)
    got = query(ren, rays, p)  # all start rays in one batch
    sums = rr.fold(got["colour"], p)
    if golden:
        entry = next(c for c in MAN["cases"] if c["name"] == golden)
        assert sums.tobytes() == golden_data.sums(entry).tobytes()
    assert sums.tobytes() == ren.render_sums(p).tobytes()
    assert (got["flags"] & ENDS != 0).all() and (got["segments"] >= 1).all()
    trace, counts = ren.render_trace(p, 1)
    assert np.ascontiguousarray(trace.reshape(-1, 6)[:, 0:3]).tobytes() == rays["origin"].tobytes()
    assert np.ascontiguousarray(trace.reshape(-1, 6)[:, 3:6]).tobytes() == rays["direction"].tobytes()
    extra = counts.reshape(-1).astype(np.int64) - got["segments"]  # (the depth-0 call runs no hit)
    assert ((extra == 0) | ((extra == 1) & (got["flags"] & rr.DEPTH != 0))).all()
    if cam.lens_radius > 0:
        assert (rays["skip"] > 8).any()


# ---- 3. deep paths --------------------------------------------------------------------------------

@pytest.mark.parametrize("rng", [MT, X128], ids=["mt", "x128"])
def test_deep_paths(ren, rng):
    sph, p = refscenes.walls2(), edge_inputs.deep_params(edge_inputs.FP64, rng)
    ren.set_scene(sph, CAM)
    ys, xs, ss = rr.all_samples(p)
    colour, draws = oracle_samples(sph, CAM, p, ys, xs, ss)
    assert (draws > 1248).sum() >= 3 and draws.max() > 1872  # several twists of the scratch engine
    got = query(ren, all_rays(CAM, p), p, count_work=True)
    assert got["colour"].tobytes() == colour.tobytes()
    assert (got["words"] == draws).all()
    fb = (got["flags"] & rr.FALLBACK) != 0
    assert (fb == ((draws > rr.LAZY_WORDS) if rng == MT else np.zeros(len(draws), bool))).all()
    assert got["segments"].max() > 200  # past the attenuation ids kept in registers, by far
    st = ren.radiance_stats()
    assert st["rays"] == len(got) and st["words"] == int(draws.sum()) and st["segments"] == int(got["segments"].sum())
    assert st["mt_fallbacks"] == int(fb.sum()) and st["out_of_domain"] == 0


# ---- 4. skip --------------------------------------------------------------------------------------

@pytest.mark.parametrize("skip", [0, 1, 4, 226, 227, 228, 623, 624, 1000])
def test_skip_discards_words(ren, skip):
    sph = refscenes.mixed12()
    ren.set_scene(sph, CAM)
    o, d = cast_ref.pixel_rays(CAM, 8, 8)
    for rng in (MT, X128):
        rays = rr.make_rays(o, d, 90000 + np.arange(64), skip)
        got = ren.radiance_rays(rays, 50, records.T_MIN, rng)
        same(got, rr.radiance(sph, rays, 50, records.T_MIN, rng), f"skip {skip} rng {rng}")
        assert (got["words"] >= skip).all() and (got["words"] > skip).any()


# ---- 5. arbitrary rays and every ending -----------------------------------------------------------

def absorbing_scene():
    """a fuzz-1 metal sphere on a ground sphere, for rays that graze the metal"""
    return [lambertian((0, -100.5, -1), 100.0, (0.8, 0.8, 0.0)), metal((0, 0, -1), 0.5, (0.8, 0.6, 0.2), 1.0)]


def traced_scenes():
    return [("glass48",) + tuple(edge_inputs.golden_scene("glass48")), ("mixed12", refscenes.mixed12(), CAM)]


@pytest.mark.parametrize("name,sph,cam", traced_scenes(), ids=[c[0] for c in traced_scenes()])
def test_arbitrary_rays(ren, name, sph, cam):
    sph = list(sph)
    ren.set_scene(sph, cam)
    cap = 8
    trace, counts = ren.render_trace(make_params(16, 9, 1, 50, 404), cap)
    trace, counts = trace.reshape(-1, cap, 6), np.minimum(counts.reshape(-1), cap)
    later = (np.arange(cap)[None, :] >= 1) & (np.arange(cap)[None, :] < counts[:, None])
    flat = trace[later]  # second and later rays: origins on surfaces and inside glass
    flat = flat[:: max(1, len(flat) // 120)][:120]
    assert len(flat) >= 100
    ends = set()
    for depth in (50, 2):
        for rng in (MT, X128):
            rays = rr.make_rays(flat[:, 0:3], flat[:, 3:6], 1000 + np.arange(len(flat)))
            want = rr.radiance(sph, rays, depth, records.T_MIN, rng)
            same(ren.radiance_rays(rays, depth, records.T_MIN, rng), want, f"{name} depth {depth} rng {rng}")
            ends |= set((want["flags"] & ENDS).tolist())
    assert ends >= {rr.SKY, rr.DEPTH}, ends  # (the golden scenes absorb nothing: the next test does)
    if name == "glass48":
        glass = [i for i, s in enumerate(sph) if s.material == records.MATERIAL_DIELECTRIC]
        assert np.isin(want["id_first"], glass).sum() > 5


def test_absorbed_paths(ren):
    sph = absorbing_scene()
    ren.set_scene(sph, CAM)
    n = 48
    o = np.stack([np.full(n, -2.0), 0.5 - 0.5 * np.linspace(0.0005, 0.05, n), np.full(n, -1.0)], 1)
    d = np.tile([1.0, 0.0, 0.0], (n, 1))
    # (spread seeds: xor128 engines whose seeds differ in a few low bits draw alike at first)
    seeds = ((7000 + np.arange(n, dtype=np.uint64)) * 2654435761 % 2 ** 32).astype(np.uint32)
    for rng in (MT, X128):
        rays = rr.make_rays(o, d, seeds)
        want = rr.radiance(sph, rays, 50, records.T_MIN, rng)
        ends = want["flags"] & ENDS
        assert (ends == rr.ABSORBED).sum() >= 3 and (ends == rr.SKY).sum() >= 3
        absorbed = want[ends == rr.ABSORBED]
        assert not absorbed["colour"].any() and (absorbed["id_last"] == 1).all()
        same(ren.radiance_rays(rays, 50, records.T_MIN, rng), want, f"absorbed rng {rng}")


# ---- 6. ragged batches ----------------------------------------------------------------------------

def test_ragged_batches_and_refill(ren):
    sph, cam = edge_inputs.golden_scene("final48")
    ren.set_scene(sph, cam)
    W, H = 200, 112
    p1 = make_params(W, H, 1, 50, 404)
    ys, xs, ss = rr.all_samples(p1)
    small = yk.camera_sample_rays(cam, p1, ys[:257], xs[:257], ss[:257])
    colour, draws = oracle_samples(sph, cam, p1, ys[:257], xs[:257], ss[:257])
    full = query(ren, small, p1)
    for n in (1, 63, 64, 65, 255, 257):
        got = query(ren, small[:n], p1)
        same(got, full[:n], f"batch of {n}")
        assert got["colour"].tobytes() == colour[:n].tobytes() and (got["words"] == draws[:n]).all()
        assert ren.radiance_stats()["rays"] == n
    lanes = ren.radiance_stats()["lanes"]
    assert lanes >= 256 and lanes % 256 == 0
    spp = lanes // (W * H) + 1
    p = make_params(W, H, spp, 50, 404)
    rays = all_rays(cam, p)
    assert len(rays) > lanes  # lanes refill
    got = query(ren, rays, p)
    _, want, _, _ = oracle_lib.render(records.sphere_array(list(sph)), cam, p, want_rgb=False, want_sums=True)
    assert rr.fold(got["colour"], p).tobytes() == want.tobytes()
    assert ren.radiance_stats()["rays"] == len(rays) and ren.radiance_stats()["lanes"] == lanes
    # a record depends on its ray alone: a permuted batch gives the permuted records
    perm = np.random.default_rng(3).permutation(4096)
    same(query(ren, rays[:4096][perm], p), got[:4096][perm], "permutation")


def test_the_chunk_seam(ren):
    """a batch past the staging chunk: a second pair of launches, the claim counter reset between"""
    chunk = 1 << 22  # yk_host_internal.hpp kRadChunk
    sph, cam = edge_inputs.golden_scene("rtiow5")
    ren.set_scene(sph, cam)
    p = make_params(64, 36, 2, 50, 404)
    base = all_rays(cam, p)
    want = query(ren, base, p)
    reps = chunk // len(base) + 1
    rays = np.tile(base, reps)[: chunk + 3]
    assert len(rays) == chunk + 3
    got = query(ren, rays, p)
    assert got.tobytes() == np.tile(want, reps)[: chunk + 3].tobytes()
    assert ren.radiance_stats()["rays"] == chunk + 3


# ---- 7. guards ------------------------------------------------------------------------------------

def test_linear_scan_gives_the_same_bytes(ren):
    sph, cam = edge_inputs.golden_scene("final48")
    ren.set_scene(sph, cam)
    p = make_params(32, 18, 4, 50, 404)
    rays = all_rays(cam, p)
    tree = query(ren, rays, p, count_work=True)
    assert ren.radiance_stats()["scan_segments"] == 0
    same(query(ren, rays, p, linear_scan=True, count_work=True), tree, "linear scan")
    st = ren.radiance_stats()
    assert st["scan_segments"] == st["segments"] == int(tree["segments"].sum())


def test_origins_either_side_of_the_trees_bound(ren):
    sph = refscenes.dupes()
    ren.set_scene(sph, CAM)
    ob = edge_inputs.origin_bound(sph, CAM)
    g = np.random.default_rng(11)
    n = 64
    axis, sign, beyond = g.integers(0, 3, n), g.choice([-1.0, 1.0], n), np.arange(n) % 2 == 1
    dist = np.where(beyond, np.nextafter(ob, INF) * g.choice([1.0, 1.5, 64.0], n), ob * g.choice([1.0, 0.99, 0.5], n))
    o = g.uniform(-0.4, 0.4, (n, 3))
    o[np.arange(n), axis] = sign * dist
    d = (np.array([0.0, 0.0, -1.0]) + g.uniform(-0.6, 0.6, (n, 3))) - o
    rays = rr.make_rays(o, d, 500 + np.arange(n))
    want = rr.radiance(sph, rays)
    got = ren.radiance_rays(rays, count_work=True)
    same(got, want, "far origins")
    assert ren.radiance_stats()["scan_segments"] >= int(beyond.sum())
    assert (want["id_first"] == 6).any() and (want["segments"] > 1).sum() > 10  # ties go to the later index


@pytest.mark.parametrize("name,k", [("final48", 14), ("final48", 18), ("rtiow5", -60), ("rtiow5", -72)])
def test_scaled_scenes_across_the_host_guard(ren, name, k):
    sph, cam = edge_inputs.scaled(*edge_inputs.golden_scene(name), k)
    ren.set_scene(sph, cam)
    p = make_params(16, 9, 2, 50, 404, t_min=edge_inputs.t_min_for(k))
    ys, xs, ss = rr.all_samples(p)
    colour, draws = oracle_samples(sph, cam, p, ys, xs, ss)
    got = query(ren, all_rays(cam, p), p, count_work=True)
    assert got["colour"].tobytes() == colour.tobytes() and (got["words"] == draws).all()
    st = ren.radiance_stats()
    in_range = edge_inputs.f64_tree_in_range(sph, cam)
    assert in_range == (k in (14, -60))
    assert (st["scan_segments"] == st["segments"]) != in_range
    same(got[::9], rr.radiance(sph, all_rays(cam, p)[::9], 50, p.t_min, MT), f"{name} k{k}")


# ---- 8. domain and arguments ----------------------------------------------------------------------

def test_rays_outside_the_domain_do_not_void_a_batch(ren):
    sph = refscenes.mixed12()
    ren.set_scene(sph, CAM)
    o, d = cast_ref.pixel_rays(CAM, 16, 9)
    o, d = o.copy(), d.copy()
    bad = {3: ("d", (NAN, 0.0, -1.0)), 17: ("d", (INF, 0.0, -1.0)), 40: ("d", (0.0, 0.0, 0.0)), 64: ("o", (2.0 ** 501, 0.0, 0.0)),
           65: ("o", (0.0, -2.0 ** 600, 0.0)), 100: ("d", (0.0, -0.0, 2.0 ** -501)), 143: ("o", (NAN, 0.0, 0.0)),
           77: ("d", (2.0 ** 501, 1.0, 1.0))}
    for i, (which, v) in bad.items():
        (o if which == "o" else d)[i] = v
    for rng in (MT, X128):
        rays = rr.make_rays(o, d, 300 + np.arange(len(o)), 5)
        want = rr.radiance(sph, rays, 50, records.T_MIN, rng)
        got = ren.radiance_rays(rays, 50, records.T_MIN, rng)
        same(got, want, "mixed batch")
        ood = np.zeros(1, records.RADIANCE_DTYPE)
        ood["id_first"] = ood["id_last"] = records.NO_HIT_ID
        ood["flags"] = rr.OOD
        for i in bad:
            assert got[i : i + 1].tobytes() == ood.tobytes(), i
        good = np.setdiff1d(np.arange(len(o)), list(bad))
        assert (got["flags"][good] & rr.OOD == 0).all() and (got["words"][good] >= 5).all()
        assert ren.radiance_stats()["out_of_domain"] == len(bad) and ren.radiance_stats()["rays"] == len(o)


def test_error_codes(ren):
    lib = yk.load_library()
    ray, rec = records.PathRay(), np.zeros(1, records.RADIANCE_DTYPE)
    ray.direction[2] = -1.0

    def par(max_depth=50, rng=MT, flags=0, reserved=0, t_min=0.001, reserved1=0):
        return ctypes.byref(records.RadianceParams(max_depth, rng, flags, reserved, t_min, reserved1))

    r, o = ctypes.byref(ray), rec.ctypes.data
    with yk.Renderer(0) as fresh:
        assert lib.ykgpu_radiance_rays(fresh._ctx, par(), r, 1, o) == YK_ERR_NO_SCENE
        assert lib.ykgpu_radiance_rays_async(fresh._ctx, par(), 16, 1, 16, None) == YK_ERR_NO_SCENE
        assert lib.ykgpu_radiance_rays(fresh._ctx, par(), None, 0, None) == 0
    ren.set_scene(refscenes.ref4(), CAM)
    ctx = ren._ctx
    assert lib.ykgpu_radiance_rays(ctx, par(), r, 1, o) == 0 and rec["flags"][0] & ENDS
    assert lib.ykgpu_radiance_rays(ctx, par(), None, 0, None) == 0
    assert lib.ykgpu_radiance_rays_async(ctx, par(), None, 0, None, None) == 0
    assert lib.ykgpu_radiance_rays(None, par(), r, 1, o) == YK_ERR_INVALID
    assert lib.ykgpu_radiance_rays(ctx, None, r, 1, o) == YK_ERR_INVALID
    assert lib.ykgpu_radiance_rays(ctx, par(), None, 1, o) == YK_ERR_INVALID
    assert lib.ykgpu_radiance_rays(ctx, par(), r, 1, None) == YK_ERR_INVALID
    assert lib.ykgpu_radiance_rays(ctx, par(flags=4), r, 1, o) == YK_ERR_INVALID
    assert b"flag" in lib.ykgpu_last_error()
    for depth in (0, 65536):
        assert lib.ykgpu_radiance_rays(ctx, par(max_depth=depth), r, 1, o) == YK_ERR_INVALID
    assert lib.ykgpu_radiance_rays(ctx, par(max_depth=65535), r, 1, o) == 0
    for t in (-0.001, INF, NAN):
        assert lib.ykgpu_radiance_rays(ctx, par(t_min=t), r, 1, o) == YK_ERR_INVALID
    assert lib.ykgpu_radiance_rays(ctx, par(t_min=0.0), r, 1, o) == 0
    assert lib.ykgpu_radiance_rays(ctx, par(rng=2), r, 1, o) == YK_ERR_UNSUPPORTED
    assert lib.ykgpu_radiance_rays_async(ctx, par(), None, 1, None, None) == YK_ERR_INVALID
    assert lib.ykgpu_radiance_rays_async(ctx, par(), 8, 1, 16, None) == YK_ERR_INVALID  # (not 16-byte aligned)
    assert lib.ykgpu_radiance_get_stats(ctx, None) == YK_ERR_INVALID
    with pytest.raises(yk.YkError):
        ren.radiance(np.zeros((2, 3)), np.zeros((3, 3)), 1)


# ---- 9. plumbing ----------------------------------------------------------------------------------

def test_device_tensors_on_torchs_stream(ren):
    torch = pytest.importorskip("torch")
    sph, cam = edge_inputs.golden_scene("final48")
    ren.set_scene(sph, cam)
    p = make_params(32, 18, 4, 50, 404)
    rays = all_rays(cam, p)
    n = len(rays)
    side = torch.cuda.Stream()
    for rng in (MT, X128):
        host = ren.radiance_rays(rays, 50, records.T_MIN, rng)
        with torch.cuda.stream(side):  # torch's current stream: the tensors are made and queried on it
            t_rays = torch.from_numpy(rays.view(np.float64).reshape(n, 8)).cuda()
            t_out = torch.full((n, 8), -7.25, dtype=torch.float64, device="cuda")
            stream = torch.cuda.current_stream()
            assert stream.cuda_stream == side.cuda_stream != 0
            ren.radiance_device(t_rays.data_ptr(), n, t_out.data_ptr(), 50, records.T_MIN, rng, stream_ptr=stream.cuda_stream)
            stream.synchronize()
        assert t_out.cpu().numpy().tobytes() == host.tobytes()
    assert ren.radiance_stats()["rays"] == n  # (the asynchronous queries record nothing)


def test_a_query_between_two_film_chunks_leaves_the_film_alone(ren):
    sph = refscenes.mixed12()
    ren.set_scene(sph, CAM)
    p = make_params(32, 18, 8, 50, 404)
    want = ren.render_sums(p)
    rays = all_rays(CAM, p)
    with ren.film(p) as film:
        film.accumulate(3)
        got = query(ren, rays, p)
        film.accumulate(5)
        sums, _, done = film.read()
    assert done == 8 and sums.tobytes() == want.tobytes()
    assert rr.fold(got["colour"], p).tobytes() == want.tobytes()


def test_a_query_after_a_second_set_scene_answers_for_the_new_scene(ren):
    p = make_params(16, 9, 2, 50, 404)
    rays = all_rays(CAM, p)
    ren.set_scene(refscenes.ref4(), CAM)
    first = query(ren, rays, p)
    ren.set_scene(refscenes.mixed12(), CAM)
    second = query(ren, rays, p)
    assert rr.fold(second["colour"], p).tobytes() == ren.render_sums(p).tobytes()
    assert first.tobytes() != second.tobytes()
    ren.set_scene(refscenes.ref4(), CAM)
    same(query(ren, rays, p), first, "back to the first scene")
    before = ren.stats()["device_bytes"]
    assert before >= ren.radiance_stats()["lanes"] * (624 * 4 + 50 * 2)  # the scratch is counted
