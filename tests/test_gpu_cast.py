"""ykgpu_cast_rays on the MI355X (include/ykgpu.h "ray queries"): every record compared byte for byte,
with no tolerance, with the numpy restatement of the definition (cast_ref); where a record holds a
NaN any payload counts as equal (the chosen inputs produce none, which each test asserts through
plain byte equality first).

The inputs are the smallest that take every path of the kernel: camera rays (coherent), the path
kernel's own traced rays (origins on surfaces and inside glass, pinned by the reference's output),
coincident spheres (ties), origins either side of the tree's bound, per-ray limits, grazing rays, zero
direction components on and beside box planes, scenes and directions scaled across the host guard
and the per-ray guards, a tree read from a large scene, rays outside the domain, batch sizes around a
wave, a block and the staging chunk, device memory on torch's stream, and a cast between two film
chunks."""
import ctypes

import numpy as np
import pytest

import cast_ref
import edge_inputs
import film_features_ref as ffr
import refscenes
import uecraytracing_amd as yk
from uecraytracing_amd import records
from uecraytracing_amd.records import make_params

pytestmark = pytest.mark.gpu

CAM = refscenes.reference_camera()
W, H = 64, 36
INF = float("inf")
NAN = float("nan")
YK_ERR_INVALID, YK_ERR_NO_SCENE = 1, 5
CHUNK = 1 << 22  # yk_cast.hpp kChunk


@pytest.fixture(scope="module")
def ren():
    r = yk.Renderer(0)
    yield r
    r.close()


def is_hit(rec):
    return (rec["flags"] & records.HIT_HIT) != 0


def check(ren, scene, o, d, t_min=records.T_MIN, t_max=INF, what="", modes=("closest", "any", "scan"), nan_free=True):
    """Casts (o, d) in the given modes and compares each with the yardstick; returns the closest-mode
    records and the yardstick's."""
    want = cast_ref.cast(scene, o, d, t_min, t_max)
    # any-hit by its definition: YK_HIT_HIT exactly when closest mode reports a hit, else as a miss
    want_any = np.zeros(len(want), records.HIT_DTYPE)
    want_any["id"] = records.NO_HIT_ID
    want_any["flags"] = np.where(want["flags"] == records.HIT_OUT_OF_DOMAIN, want["flags"], want["flags"] & records.HIT_HIT)
    got = None
    for mode in modes:
        kw = dict(any_hit=mode == "any", linear_scan=mode in ("scan", "scan-any"))
        if mode == "scan-any":
            kw["any_hit"] = True
        rec = ren.cast_rays(o, d, t_min, t_max, **kw)
        ref = want_any if kw["any_hit"] else want
        if nan_free:
            bad = int((rec.view(np.uint64).reshape(-1, 8) != ref.view(np.uint64).reshape(-1, 8)).any(1).sum())
            assert rec.tobytes() == ref.tobytes(), f"{what} {mode}: {bad} of {len(ref)} records differ"
        else:
            assert cast_ref.same_bytes(rec, ref), f"{what} {mode}"
        st = ren.cast_stats()
        assert st["rays"] == len(ref) and st["hits"] == int(is_hit(ref).sum()), (what, mode, st)
        assert st["out_of_domain"] == int((ref["flags"] == records.HIT_OUT_OF_DOMAIN).sum())
        if mode.startswith("scan"):
            assert st["scan_rays"] == st["rays"] - st["out_of_domain"]
        assert st["node_visits"] == 0 and st["sphere_tests"] == 0 and st["kernel_ms"] > 0 and st["total_ms"] > 0
        if mode == "closest":
            got = rec
    return got, want


# ---- 1. camera rays -------------------------------------------------------------------------------

def camera_cases():
    f48, c48 = edge_inputs.golden_scene("final48")
    rt5, c5 = edge_inputs.golden_scene("rtiow5")
    return [("final48", f48, c48), ("rtiow5", rt5, c5), ("shell", ffr.shell(), CAM), ("many40", ffr.many(40), CAM)]


@pytest.mark.parametrize("name,scene,cam", camera_cases(), ids=[c[0] for c in camera_cases()])
def test_camera_rays(ren, name, scene, cam):
    ren.set_scene(scene, cam)
    o, d = cast_ref.pixel_rays(cam, W, H)
    got, want = check(ren, scene, o, d, what=name, modes=("closest", "any", "scan", "scan-any"))
    assert 0.2 < is_hit(want).mean() <= 1.0
    if name == "final48":
        assert 0.80 < is_hit(want).mean() < 0.86 and len(np.unique(want["id"][is_hit(want)])) >= 30
        ren.cast_rays(o, d)
        assert ren.cast_stats()["scan_rays"] == 0
        counted = ren.cast_rays(o, d, count_work=True)
        st = ren.cast_stats()
        assert counted.tobytes() == want.tobytes()
        assert st["node_visits"] >= st["rays"]
        assert 0 < st["sphere_tests"] < st["rays"] * len(scene) / 4, st  # the tree really culls
        ren.cast_rays(o, d, linear_scan=True, count_work=True)
        assert ren.cast_stats()["sphere_tests"] == len(o) * len(scene) and ren.cast_stats()["node_visits"] == 0


# ---- 2. against the feature kernel ----------------------------------------------------------------

def test_cast_equals_the_feature_pass(ren):
    scene, cam = edge_inputs.golden_scene("final48")
    ren.set_scene(scene, cam)
    with ren.film(make_params(W, H, 2, 50, 404)) as film:
        mean, _, _ = film.features(1)
    o, d = cast_ref.pixel_rays(cam, W, H)
    got = ren.cast_rays(o, d)
    f = mean.reshape(-1, 7)
    assert np.ascontiguousarray(f[:, 3:6]).tobytes() == got["normal"].tobytes()
    assert np.ascontiguousarray(f[:, 6]).tobytes() == got["t"].tobytes()
    miss = ~is_hit(got)
    assert miss.any() and not f[miss, 3:7].any() and not got["p"][miss].any()


# ---- 3. path rays pinned by the reference ---------------------------------------------------------

def traced_cases():
    return [("mixed12", refscenes.mixed12(), CAM), ("glass48",) + tuple(edge_inputs.golden_scene("glass48")),
            ("final48",) + tuple(edge_inputs.golden_scene("final48")), ("dupes", refscenes.dupes(), CAM)]


@pytest.mark.parametrize("name,scene,cam", traced_cases(), ids=[c[0] for c in traced_cases()])
def test_path_rays_hit_where_their_successors_start(ren, name, scene, cam):
    ren.set_scene(scene, cam)
    cap = 16
    rays, counts = ren.render_trace(make_params(16, 9, 4, 50, 404), cap)
    rays, counts = rays.reshape(-1, cap, 6), np.minimum(counts.reshape(-1), cap)
    k = np.arange(cap)[None, :]
    recorded = k < counts[:, None]
    has_next = (k + 1) < counts[:, None]
    flat = rays[recorded]
    got, want = check(ren, scene, flat[:, 0:3], flat[:, 3:6], 0.001, INF, what=name)
    # a scatter leaves from rec.p (material.hpp), and the trace is pinned to the reference's output
    pos = np.cumsum(recorded.reshape(-1)).reshape(recorded.shape) - 1
    src, nxt = pos[has_next], pos[np.roll(has_next, 1, axis=1) & recorded & (k > 0)]
    assert len(src) == len(nxt) == int(has_next.sum())
    assert is_hit(got[src]).all(), f"{name}: {int((~is_hit(got[src])).sum())} scattered rays miss"
    assert got["p"][src].tobytes() == np.ascontiguousarray(flat[nxt, 0:3]).tobytes()
    assert len(src) >= 0.5 * len(flat), (len(src), len(flat))


# ---- 4. ties and far origins ----------------------------------------------------------------------

def test_ties_go_to_the_later_index_and_far_origins_take_the_scan(ren):
    scene = refscenes.dupes()
    ren.set_scene(scene, CAM)
    o, d = cast_ref.pixel_rays(CAM, W, H)
    got, want = check(ren, scene, o, d, what="dupes")
    ids = set(np.unique(want["id"]).tolist())
    assert ids == {records.NO_HIT_ID, 0, 6, 7}, ids
    assert 0.10 < (want["id"] == 6).mean() < 0.20
    # origins either side of the tree's bound, aimed at the coincident spheres and past them
    ob = edge_inputs.origin_bound(scene, CAM)
    rng = np.random.default_rng(11)
    n = 192
    axis = rng.integers(0, 3, n)
    sign = rng.choice([-1.0, 1.0], n)
    beyond = np.arange(n) % 2 == 1
    dist = np.where(beyond, np.nextafter(ob, INF) * rng.choice([1.0, 1.5, 64.0], n), ob * rng.choice([1.0, 0.99, 0.5], n))
    fo = rng.uniform(-0.4, 0.4, (n, 3))
    fo[np.arange(n), axis] = sign * dist
    target = np.array([0.0, 0.0, -1.0]) + rng.uniform(-0.6, 0.6, (n, 3))
    fd = target - fo
    assert (np.abs(fo).max(1) > ob).sum() == beyond.sum() == n // 2
    got, want = check(ren, scene, fo, fd, 0.001, INF, what="far origins", modes=("closest", "any"))
    ren.cast_rays(fo, fd, 0.001, INF)
    assert ren.cast_stats()["scan_rays"] == int(beyond.sum())
    assert 0.3 < is_hit(want).mean() and (want["id"][is_hit(want)] == 6).any()


# ---- 5. limits ------------------------------------------------------------------------------------

def test_per_ray_limits(ren):
    scene, cam = edge_inputs.golden_scene("final48")
    ren.set_scene(scene, cam)
    rng = np.random.default_rng(5)
    n = 4096
    ext = max(max(abs(c) for c in s.center) for s in scene[1:])
    o = rng.uniform(-1.0, 1.0, (n, 3)) * np.array([ext, 0.0, ext]) + np.array([0.0, 0.0, 0.0])
    o[:, 1] = rng.uniform(0.05, 2.0, n)
    d = rng.normal(size=(n, 3))
    d[:, 1] *= 0.25
    t_min = rng.choice([0.0, 0.001, 0.5], n)
    t_max = np.where(np.arange(n) % 2 == 1, 1.5, INF)
    got, want = check(ren, scene, o, d, t_min, t_max, what="limits")
    free = cast_ref.cast(scene, o, d, 0.0, INF)
    changed = int((want.view(np.uint64).reshape(-1, 8) != free.view(np.uint64).reshape(-1, 8)).any(1).sum())
    assert changed > 200 and is_hit(want).mean() < is_hit(free).mean() - 0.05
    lim = t_max < INF
    assert (want["t"][lim & is_hit(want)] <= 1.5).all() and (want["t"][is_hit(want)] >= t_min[is_hit(want)]).all()
    assert is_hit(want)[lim].mean() > 0.1 and len(np.unique(want["id"][is_hit(want)])) > 20


# ---- 6. culling edges -----------------------------------------------------------------------------

def test_grazing_camera_rays(ren):
    scene = refscenes.graze()
    ren.set_scene(scene, CAM)
    o, d = cast_ref.pixel_rays(CAM, W, H)
    _, want = check(ren, scene, o, d, what="graze")
    assert len(np.unique(want["id"][is_hit(want)])) >= 3 and not is_hit(want).all()


@pytest.mark.parametrize("name", ["mixed12", "rtiow5"])
def test_zero_direction_components_on_and_beside_box_planes(ren, name):
    scene = refscenes.mixed12() if name == "mixed12" else edge_inputs.golden_scene(name)[0]
    cams = [edge_inputs.planar_camera(a) for a in edge_inputs.PLANAR_AXES]
    ren.set_scene(scene, cams[0])
    os_, ds = [], []
    for axis, cam in zip(edge_inputs.PLANAR_AXES, cams):
        o, d = cast_ref.pixel_rays(cam, edge_inputs.PLANAR_W, edge_inputs.PLANAR_H)
        k = 1 if axis == "y" else 0
        assert not d[:, k].any() and np.signbit(d[:, k]).all() == (axis == "x-negzero")
        # the planes of the spheres' boxes along the zero axis, and their neighbours either side
        planes = sorted({s.center[k] + sg * abs(s.radius) for s in scene[:6] for sg in (-1.0, 1.0)} | {0.0})
        for pl in planes:
            if abs(pl) > 50:
                continue
            for x in (np.nextafter(pl, -INF), pl, np.nextafter(pl, INF)):
                oo = o.copy()
                oo[:, k] = x
                os_.append(oo)
                ds.append(d)
    o, d = np.concatenate(os_), np.concatenate(ds)
    _, want = check(ren, scene, o, d, what=f"planar {name}", modes=("closest", "any"))
    ren.cast_rays(o, d)
    assert ren.cast_stats()["scan_rays"] == len(o)  # a zero component: the slab test cannot serve it
    assert 0.2 < is_hit(want).mean() and len(np.unique(want["id"][is_hit(want)])) >= 3


@pytest.mark.parametrize("k", [-240, -76, -60, 12, 18, 240])
def test_scaled_scenes_across_the_host_guard(ren, k):
    for name in ("rtiow5", "final48"):
        scene, cam = edge_inputs.scaled(*edge_inputs.golden_scene(name), k)
        ren.set_scene(scene, cam)
        o, d = cast_ref.pixel_rays(cam, 32, 18)
        _, want = check(ren, scene, o, d, edge_inputs.t_min_for(k), INF, what=f"{name} 2^{k}", modes=("closest", "any"))
        ren.cast_rays(o, d, edge_inputs.t_min_for(k), INF)
        st = ren.cast_stats()
        assert st["out_of_domain"] == 0 and is_hit(want).mean() > 0.5
        if not edge_inputs.f64_tree_in_range(scene, cam):
            assert st["scan_rays"] == st["rays"]  # the host guard: every ray takes the scan


@pytest.mark.parametrize("k", [-480, -250, 30, 199])
def test_scaled_directions(ren, k):
    scene = refscenes.mixed12()
    cam = edge_inputs.direction_scaled(CAM, k)
    ren.set_scene(scene, cam)
    o, d = cast_ref.pixel_rays(cam, 32, 18)
    t_min = 0.001 * 2.0 ** -k
    _, want = check(ren, scene, o, d, t_min, INF, what=f"directions 2^{k}", modes=("closest", "any"))
    assert ren.cast_stats()["out_of_domain"] == 0 and is_hit(want).mean() > 0.5
    unit = cast_ref.cast(scene, *cast_ref.pixel_rays(CAM, 32, 18), 0.001, INF)
    assert (want["id"] == unit["id"]).mean() > 0.99  # (the same picture: scaling d scales t)


def test_large_scene_read_from_global_memory(ren):
    import random
    from uecraytracing_amd.records import dielectric, lambertian, metal
    rng = random.Random(5)
    s = [lambertian((0, -1000.5, -1), 1000.0, (0.5, 0.5, 0.5))]
    for _ in range(2600):
        c = (rng.uniform(-6, 6), rng.uniform(-0.5, 3), rng.uniform(-9, -1))
        k = rng.random()
        r = rng.uniform(0.03, 0.15)
        if k < 0.6:
            s.append(lambertian(c, r, (rng.random(), rng.random(), rng.random())))
        elif k < 0.85:
            s.append(metal(c, r, (rng.random(), rng.random(), rng.random()), rng.choice([0.0, 0.2])))
        else:
            s.append(dielectric(c, r, 1.5))
    ren.set_scene(s, CAM)
    o, d = cast_ref.pixel_rays(CAM, 32, 16)
    o, d = np.concatenate([o, o + np.array([0.3, 1.0, -4.0])]), np.concatenate([d, d * np.array([1.0, -1.0, 1.0])])
    assert len(o) == 1024
    _, want = check(ren, s, o, d, what="2601 spheres")
    assert len(np.unique(want["id"][is_hit(want)])) > 50
    ren.cast_rays(o, d, count_work=True)
    st = ren.cast_stats()
    assert st["scan_rays"] == 0 and st["sphere_tests"] < st["rays"] * len(s) / 4


# ---- 7. domain and shape --------------------------------------------------------------------------

def test_rays_outside_the_domain_do_not_void_a_batch(ren):
    scene = refscenes.mixed12()
    ren.set_scene(scene, CAM)
    o, d = cast_ref.pixel_rays(CAM, 16, 9)
    n = len(o)
    t_min, t_max = np.full(n, 0.001), np.full(n, INF)
    good = ren.cast_rays(o, d, t_min, t_max)
    o2, d2 = o.copy(), d.copy()
    bad = np.arange(5, n, 7)[:12]
    o2[bad[0], 0] = NAN
    d2[bad[1], 2] = NAN
    o2[bad[2], 1] = INF
    d2[bad[3], 0] = -INF
    d2[bad[4]] = 0.0
    d2[bad[5]] = (-0.0, 0.0, -0.0)
    t_min[bad[6]] = -1e-300
    t_min[bad[7]], t_max[bad[7]] = 2.0, 1.0
    t_max[bad[8]] = NAN
    d2[bad[9]] = d2[bad[9]] * 2.0 ** 520
    d2[bad[10]] = d2[bad[10]] * 2.0 ** -520
    t_min[bad[11]] = INF
    got, want = check(ren, scene, o2, d2, t_min, t_max, what="domain", modes=("closest", "any", "scan"))
    assert (got["flags"][bad] == records.HIT_OUT_OF_DOMAIN).all() and (got["id"][bad] == records.NO_HIT_ID).all()
    assert not got["p"][bad].any() and not got["normal"][bad].any() and not got["t"][bad].any()
    rest = np.setdiff1d(np.arange(n), bad)
    assert got[rest].tobytes() == good[rest].tobytes() and is_hit(good[rest]).mean() > 0.5
    assert ren.cast_stats()["out_of_domain"] == len(bad)


def test_batch_sizes_and_the_chunk_seam(ren):
    scene = refscenes.ref4()
    ren.set_scene(scene, CAM)
    o, d = cast_ref.pixel_rays(CAM, 32, 18)
    want = cast_ref.cast(scene, o, d)
    for n in (0, 1, 63, 64, 65, 257):
        got = ren.cast_rays(o[:n], d[:n])
        assert got.tobytes() == want[:n].tobytes(), n
        if n:
            assert ren.cast_stats()["rays"] == n
    # the staging chunk's seam, against the same rays cast in two halves
    n = CHUNK + 3
    idx = np.arange(n) % len(o)
    bo, bd = o[idx], d[idx] * (1.0 + (np.arange(n) % 5)[:, None])
    whole = ren.cast_rays(bo, bd)
    st = ren.cast_stats()
    assert st["rays"] == n and st["hits"] == int(is_hit(whole).sum())
    h = n // 2
    halves = np.concatenate([ren.cast_rays(bo[:h], bd[:h]), ren.cast_rays(bo[h:], bd[h:])])
    assert whole.tobytes() == halves.tobytes()
    k = np.r_[0:600, CHUNK - 300:CHUNK + 3]
    assert whole[k].tobytes() == cast_ref.cast(scene, bo[k], bd[k]).tobytes()
    ren.render(make_params(16, 9, 1, 50, 404))  # (a render's statistics carry the context's device bytes)
    assert ren.stats()["device_bytes"] >= CHUNK * 128


def test_error_codes(ren):
    lib = yk.load_library()
    ray, hit = records.Ray(), records.Hit()
    with yk.Renderer(0) as fresh:
        assert lib.ykgpu_cast_rays(fresh._ctx, ctypes.byref(ray), 1, 0, ctypes.byref(hit)) == YK_ERR_NO_SCENE
        assert lib.ykgpu_cast_rays_async(fresh._ctx, 8, 1, 0, 8, None) == YK_ERR_NO_SCENE
        assert lib.ykgpu_cast_rays(fresh._ctx, None, 0, 0, None) == 0
    ren.set_scene(refscenes.ref4(), CAM)
    ctx = ren._ctx
    assert lib.ykgpu_cast_rays(ctx, None, 0, 0, None) == 0
    assert lib.ykgpu_cast_rays_async(ctx, None, 0, 0, None, None) == 0
    assert lib.ykgpu_cast_rays(ctx, None, 1, 0, ctypes.byref(hit)) == YK_ERR_INVALID
    assert lib.ykgpu_cast_rays(ctx, ctypes.byref(ray), 1, 0, None) == YK_ERR_INVALID
    assert lib.ykgpu_cast_rays(ctx, ctypes.byref(ray), 1, 8, ctypes.byref(hit)) == YK_ERR_INVALID
    assert b"flag" in lib.ykgpu_last_error()
    assert lib.ykgpu_cast_rays_async(ctx, None, 1, 0, None, None) == YK_ERR_INVALID
    assert lib.ykgpu_cast_rays_async(ctx, 8, 1, 16, 8, None) == YK_ERR_INVALID
    with pytest.raises(yk.YkError):
        ren.cast_rays(np.zeros((2, 3)), np.zeros((3, 3)))


# ---- 8. device memory -----------------------------------------------------------------------------

def test_device_tensors_on_torchs_stream(ren):
    torch = pytest.importorskip("torch")
    scene, cam = edge_inputs.golden_scene("final48")
    ren.set_scene(scene, cam)
    o, d = cast_ref.pixel_rays(cam, W, H)
    n = len(o)
    host = ren.cast_rays(o, d, 0.001, INF)
    rays = np.concatenate([o, d, np.full((n, 1), 0.001), np.full((n, 1), INF)], axis=1)
    side = torch.cuda.Stream()
    for flags, ref in ((0, host), (records.CAST_ANY_HIT, ren.cast_rays(o, d, 0.001, INF, any_hit=True))):
        with torch.cuda.stream(side):  # torch's current stream: the tensors are made and cast on it
            t_rays = torch.from_numpy(rays).cuda()
            t_hits = torch.full((n, 8), -7.25, dtype=torch.float64, device="cuda")
            stream = torch.cuda.current_stream()
            assert stream.cuda_stream == side.cuda_stream != 0
            ren.cast_rays_device(t_rays.data_ptr(), n, t_hits.data_ptr(), stream.cuda_stream, flags)
            stream.synchronize()
        words = t_hits.view(torch.int32).cpu().numpy()
        assert words.tobytes() == ref.tobytes()
        assert (words[:, 14].view(np.uint32) == ref["id"]).all() and (words[:, 15].view(np.uint32) == ref["flags"]).all()
        assert t_hits.cpu().numpy()[:, 6].tobytes() == ref["t"].tobytes()
    assert ren.cast_stats()["rays"] == n  # (the asynchronous casts record nothing)


# ---- 9. coexistence -------------------------------------------------------------------------------

def test_a_cast_between_two_film_chunks_leaves_the_film_alone(ren):
    scene = refscenes.mixed12()
    ren.set_scene(scene, CAM)
    p = make_params(32, 18, 8, 50, 404)
    want = ren.render_sums(p)
    o, d = cast_ref.pixel_rays(CAM, 32, 18)
    with ren.film(p) as film:
        film.accumulate(3)
        got = ren.cast_rays(o, d)
        film.accumulate(5)
        sums, _, done = film.read()
    assert done == 8 and sums.tobytes() == want.tobytes()
    assert got.tobytes() == cast_ref.cast(scene, o, d).tobytes()
