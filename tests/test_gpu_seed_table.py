"""The seed table on the MI355X (DESIGN.md §3 "Seed table"): the first call of a key whose tile has
sky blocks walks as ever, the second consecutive one also stores every sample's x_397 (the fill
call); in the calls of that key after it the sky kernel loads the word instead of walking.  The warm-ups fill and keep walking, and
a call without a sky block neither allocates nor fills nor reads.  Every image here is compared with
the CPU oracle byte for byte (RGB8) and bit for bit (the float64 sums), whichever behaviour made it.

72x40 at 6 spp (two launches, 4 + 2; partial bottom blocks) on the scenes of
tests/test_gpu_sky_blocks.py: rtiow5 (no sky block: no table) and final48 seen by the pitched
camera (33 of 45 blocks are sky: yk_sky_samples fills and reads them, the warm-up fills the other
12), without a lens (yk_mt_warmup's instances) and with one (yk_mt_warmup_defer's).

That a reading call really reads is shown twice: device_bytes holds the table's 4 * T * spp bytes
from the fill call on, and under the test hook yk_seed_table_test (outside the C-ABI), which makes
every fill store x_397 ^ 0x80000000, the pixels of the sky blocks, and no others, come out different
(child processes, tests/seed_table_child.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import sky_blocks_lib as sbl
import test_gpu_sky_blocks as sky_cases
import uecraytracing_amd as yk
from uecraytracing_amd import tiles
from uecraytracing_amd.records import (FLAG_COUNT_WORK, PRECISION_FP32, RNG_XOR128, SEED_RANDOM_DEVICE, make_params)

gpu = pytest.mark.gpu
pytestmark = gpu

W, H, SPP, DEPTH = sky_cases.W, sky_cases.H, sky_cases.SPP, sky_cases.DEPTH
CASES = [("rtiow5", 0.0), ("rtiow5", 0.05), ("pitched", 0.0), ("pitched", 0.05)]
IDS = [f"{n}-lens{l}" for n, l in CASES]
scene, oracle, same_bits = sky_cases.scene, sky_cases.oracle, sky_cases.same_bits


def params(seed0=404, spp=SPP, **kw):
    return make_params(W, H, spp, DEPTH, seed0, **kw)


def table_bytes(p, name="pitched"):
    """the table's share of device_bytes after a call of p on scene `name`: only a view with sky blocks has one"""
    return 4 * p.row_count * p.tile_width() * p.samples_per_pixel if name == "pitched" else 0


def check(ren, name, lens, p, what=""):
    """one render and one render_sums of p against the oracle; returns device_bytes after the render"""
    rgb, sums = oracle(name, lens, p)
    np.testing.assert_array_equal(ren.render(p), rgb, err_msg=f"{name} lens {lens} {what}")
    b = ren.stats()["device_bytes"]
    assert same_bits(ren.render_sums(p), sums), f"{name} lens {lens} {what}: sums"
    return b


@pytest.fixture()
def ren():
    r = yk.Renderer(0)
    yield r
    r.close()


@pytest.fixture()
def ren_off(monkeypatch):
    """a context that keeps no table (the switch is read when the context is created)"""
    monkeypatch.setenv("YKGPU_SEED_TABLE", "0")
    r = yk.Renderer(0)
    monkeypatch.delenv("YKGPU_SEED_TABLE")
    yield r
    r.close()


@pytest.mark.parametrize("name,lens", CASES, ids=IDS)
def test_fill_read_read(ren, ren_off, name, lens):
    """Three render calls (walk, fill, read) and render_sums of one key: the oracle's bytes; with sky
    blocks the context holds 4*T*spp bytes more than one without a table from the second call on,
    and nothing more after it; without a sky block it holds what the other holds."""
    p = params()
    rgb, sums = oracle(name, lens, p)
    held = []
    for r in (ren, ren_off):
        r.set_scene(*scene(name, lens))
        b = []
        for call in range(3):
            np.testing.assert_array_equal(r.render(p), rgb, err_msg=f"call {call}")
            st = r.stats()
            assert st["launches"] == 2 and st["samples"] == W * H * SPP
            b.append(st["device_bytes"])
        assert same_bits(r.render_sums(p), sums)
        b.append(r.stats()["device_bytes"])
        np.testing.assert_array_equal(r.render(p), rgb, err_msg="after the sums")
        held.append(b)
    on, off = held
    print("device_bytes with / without the table:", on, off)
    assert [a - b for a, b in zip(on, off)] == [0] + [table_bytes(p, name)] * 3
    assert on[1] == on[2] and off[0] == off[1] == off[2]


@pytest.mark.parametrize("name,lens", CASES, ids=IDS)
def test_calls_in_flight(ren, name, lens):
    """Four calls enqueued with no synchronisation between them: the second is the fill call, the
    third and fourth read."""
    import torch
    ren.set_scene(*scene(name, lens))
    p = params()
    rgb, _ = oracle(name, lens, p)
    outs = [torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda:0") for _ in range(4)]
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    for o in outs:
        ren.render_async(p, o.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    for k, o in enumerate(outs):
        np.testing.assert_array_equal(o.cpu().numpy(), rgb, err_msg=f"call {k} in flight")
    np.testing.assert_array_equal(ren.render(p), rgb)


@pytest.mark.parametrize("lens", (0.0, 0.05))
def test_camera_and_scene_change_under_one_key(ren, lens):
    """Filled under the pitched camera, read under the level one and under the pitched one again:
    pixels cross between the sky list and the path order (33 sky blocks, then 3 or none), so each
    kernel reads words the other stored.  Then filled under one scene and read under another."""
    p = params()
    for name in ("pitched", "final48", "pitched", "rtiow5", "pitched"):
        ren.set_scene(*scene(name, lens))
        check(ren, name, lens, p, "under one key")
    p5 = params(seed0=777)
    ren.set_scene(*scene("rtiow5", lens))
    check(ren, "rtiow5", lens, p5, "filled under rtiow5")
    ren.set_scene(*scene("pitched", lens))
    check(ren, "pitched", lens, p5, "read under the pitched final48")


@pytest.mark.parametrize("name,lens", [("rtiow5", 0.05), ("pitched", 0.0), ("pitched", 0.05)],
                         ids=["rtiow5-lens", "pitched", "pitched-lens"])
def test_key_changes(ren, ren_off, name, lens):
    """Every change of the key refills (the same buffer when the size stays, another when not): seed0,
    seeds that wrap, spp, and the tiles of an N-GPU split alternating on one context.  Each key gets
    four calls (image, sums, image, sums: it walks, fills and reads twice); from the third on the
    context holds exactly the key's table more than a context without one that made the same calls."""
    ren.set_scene(*scene(name, lens))
    ren_off.set_scene(*scene(name, lens))
    keys = [params(404), params(405), params(404), params(4294967000), params(404, 6), params(404, 5),
            params(404, 6)]
    split = [params(rows=tiles.tile_rows(0, 2, H)), params(rows=tiles.tile_rows(1, 2, H)),
             params(cols=tiles.tile_cols(0, 2, W))]
    assert split[2].col_band_log2 == 3 and split[2].tile_width() == 40
    for p in keys + split + split:
        what = f"seed0 {p.seed0} spp {p.samples_per_pixel} rows {p.row_begin}::{p.row_stride} cols {p.col_count}"
        check(ren, name, lens, p, what + " (walk, fill)")
        check(ren_off, name, lens, p, what + " (no table)")
        b, b_off = check(ren, name, lens, p, what + " (read)"), check(ren_off, name, lens, p, what + " (no table)")
        assert b - b_off == table_bytes(p, name), what


@pytest.mark.parametrize("name,lens", [("rtiow5", 0.05), ("pitched", 0.05)], ids=["rtiow5-lens", "pitched-lens"])
def test_ineligible_calls_in_between(ren, name, lens):
    """FP32, xor128, random-device seeds, the counting instance and a film pass between two calls of
    one key: each renders its own oracle's image, and the table call after them still reads its
    words (they neither read nor write the table)."""
    s, c = scene(name, lens)
    ren.set_scene(s, c)
    p = params()
    check(ren, name, lens, p, "fill")  # (its render_sums brings the context's sums buffer)
    held = check(ren, name, lens, p, "read")
    assert check(ren, name, lens, p, "read again") == held
    for kw in (dict(precision=PRECISION_FP32), dict(rng=RNG_XOR128),
               dict(seed_mode=SEED_RANDOM_DEVICE, seed_key=0x0123456789ABCDEF), dict(flags=FLAG_COUNT_WORK)):
        q = params(**kw)
        check(ren, name, lens, q, f"ineligible {kw}")
        check(ren, name, lens, p, f"the table call after {kw}")
    rgb, sums = oracle(name, lens, p)
    with ren.film(p) as film:
        assert film.accumulate(SPP) == SPP
        fs, _, _ = film.read()
        assert same_bits(fs, sums)
        np.testing.assert_array_equal(film.resolve(), rgb)
    check(ren, name, lens, p, "after the film pass")


# ---- child processes: the switches, and the poisoned variant ----

def run_child(folder, env=None):
    e = dict(os.environ)
    for k in ("YKGPU_SEED_TABLE", "YKGPU_SEED_TABLE_MAX_MB", "SEED_TABLE_CHILD_POISON"):
        e.pop(k, None)
    e.update(env or {})
    pr = subprocess.run([sys.executable, os.path.join(sbl.ROOT, "tests", "seed_table_child.py"), str(folder)], env=e,
                        capture_output=True, text=True, timeout=240)
    assert pr.returncode == 0, pr.stderr[-2000:]
    with open(os.path.join(str(folder), "stats.json")) as f:
        stats = json.load(f)
    with np.load(os.path.join(str(folder), "out.npz")) as z:
        return {k: z[k] for k in z.files}, stats


@pytest.fixture(scope="module")
def child_runs(tmp_path_factory):
    """the child's calls with the table on, switched off and capped below its need, and with
    poisoned fills (table on, and switched off)"""
    runs = {}
    for tag, env in (("on", None), ("off", {"YKGPU_SEED_TABLE": "0"}), ("capped", {"YKGPU_SEED_TABLE_MAX_MB": "0"}),
                     ("poison", {"SEED_TABLE_CHILD_POISON": "1"}),
                     ("poison_off", {"SEED_TABLE_CHILD_POISON": "1", "YKGPU_SEED_TABLE": "0"})):
        runs[tag] = run_child(tmp_path_factory.mktemp("seed_table_" + tag), env)
    return runs


def child_oracles(key):
    name, lens = key.rsplit("-", 1)
    return oracle(name, float(lens), params()), oracle(name, float(lens), params(seed0=405))


@pytest.mark.parametrize("name,lens", CASES, ids=IDS)
def test_switches(child_runs, name, lens):
    """YKGPU_SEED_TABLE=0 and a cap below the need (72x40x6 needs 69120 bytes; the cap counts MB, so
    0): the oracle's bytes, and device_bytes without the table's share.  With poisoned fills and the
    switch off every call renders the oracle's bytes: nothing stores or reads a word.  (The Python
    package reads both variables when it creates the context and hands them to the library.)"""
    key = f"{name}-{lens}"
    (rgb, sums), (rgb5, sums5) = child_oracles(key)
    for tag in ("on", "off", "capped", "poison_off"):
        got, _ = child_runs[tag]
        for k, want in (("_first_rgb", rgb), ("_fill_rgb", rgb), ("_reseeded_fill_rgb", rgb5), ("_second_rgb", rgb), ("_second_sums", sums), ("_reseeded_rgb", rgb5),
                        ("_reseeded_sums", sums5)):
            assert same_bits(got[key + k], want), (tag, key + k)
    on, off, capped = (child_runs[t][1] for t in ("on", "off", "capped"))
    # (the first call of a key walks and holds no table yet; the second has filled)
    for call, share in (("_first", 0), ("_second", table_bytes(params(), name))):
        assert off[key + call] == capped[key + call] == on[key + call] - share


SKY_PIXELS = {"rtiow5": 0, "pitched": 33 * 64}  # (test_gpu_sky_blocks.SKY_BLOCKS: whole 8 x 8 blocks at 72x40)


@pytest.mark.parametrize("name,lens", CASES, ids=IDS)
def test_poisoned_fill_shows_the_read(child_runs, name, lens):
    """Under the test hook every fill stores x_397 ^ 0x80000000.  The first call of a key walks and
    the fill call, the second, uses the values it walked: the oracle's image twice.  In the calls of
    the key after them the sky kernel reads the flipped
    word: word j of a sample's engine is temper(x_(397+j) ^ mix(x_j, x_(j+1))) and the lane derives
    x_398, x_399, ... from the word it loaded by the seeding recurrence, so every word the start draws
    is another one, every sample's jitter and camera ray move, and a pixel keeps its six-sample sums
    only by coincidence: at least 99 of 100 pixels of the sky blocks must differ, and no other pixel,
    since the warm-ups walk; none at all on rtiow5, which has no sky block and no table.  After a
    seed0 change the calls walk and fill again: their own oracle's image."""
    key = f"{name}-{lens}"
    (rgb, sums), (rgb5, sums5) = child_oracles(key)
    got, _ = child_runs["poison"]
    readers = SKY_PIXELS[name]
    assert same_bits(got[key + "_first_rgb"], rgb), "the first call of a key walks"
    assert same_bits(got[key + "_fill_rgb"], rgb), "the fill call renders from its own walks"
    assert same_bits(got[key + "_reseeded_fill_rgb"], rgb5), "... and again under the new seed0"
    for k, want in (("_second_sums", sums), ("_reseeded_sums", sums5)):
        differ = int((got[key + k] != want).any(2).sum())
        print(key + k, "pixels whose sums differ from the oracle's:", differ, "of", readers, "read")
        assert 0.99 * readers <= differ <= readers, "exactly the pixels of the kernel that reads see the poisoned words"
    if readers == 0:
        assert same_bits(got[key + "_second_rgb"], rgb)
    assert same_bits(got[key + "_reseeded_rgb"], rgb5), "a new seed0 walks again"
