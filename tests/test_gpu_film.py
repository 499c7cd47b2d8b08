"""The progressive film on the MI355X (include/ykgpu.h "progressive film"): any chunking of the
samples yields the one-shot render's float64 sums and bytes — checked bit for bit, with no
tolerance, after every chunk, against the oracle's per-sample colours folded in numpy (film_ref;
tests/test_film.py shows that fold to be the one-shot render).  The shapes are the smallest at
which the mechanism can go wrong: 13 samples are the smallest count whose one-shot schedule has
two launches (4 + 9), and [5, 8] cuts inside the first launch's successor.
"""
import ctypes
import subprocess

import numpy as np
import pytest

import film_ref
import refscenes
import uecraytracing_amd as yk
from uecraytracing_amd.records import PRECISION_FP32, RNG_XOR128, SEED_RANDOM_DEVICE, make_params

pytestmark = pytest.mark.gpu

CAM = refscenes.reference_camera()


@pytest.fixture(scope="module")
def ren():
    r = yk.Renderer(0)
    yield r
    r.close()


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def fill(film, cols, chunks, after=None):
    """Accumulates `chunks` and checks the whole state after every one against the prefix fold."""
    S, Q = film_ref.prefixes(cols)
    done = 0
    for n in chunks:
        assert film.accumulate(n) == done + n
        done += n
        sums, sumsq, d = film.read()
        assert d == done == film.done
        assert same(sums, S[done]), f"sums after {done} of {chunks}"
        assert same(sumsq, Q[done]), f"second moments after {done} of {chunks}"
        assert same(film.resolve(), film_ref.to_color3b(S[done], done)), f"image after {done} of {chunks}"
        if after:
            after(done)
    return S, Q


def against_one_shot(ren, film, p):
    sums, _, done = film.read()
    assert done == p.samples_per_pixel
    assert same(sums, ren.render_sums(p))
    assert same(film.resolve(), ren.render(p))


REF4_13 = dict(width=16, height=9, spp=13, max_depth=50, seed0=404)


@pytest.mark.parametrize("chunks", [[13], [5, 8], [4, 9], [1] * 13], ids=["13", "5+8", "4+9", "13x1"])
def test_chunking_invariance(ren, chunks):
    ren.set_scene(refscenes.ref4(), CAM)
    p = make_params(**REF4_13)
    with ren.film(p) as film:
        fill(film, film_ref.colours(refscenes.ref4(), CAM, p), chunks)
        against_one_shot(ren, film, p)


@pytest.mark.parametrize("mode", [dict(precision=PRECISION_FP32), dict(rng=RNG_XOR128),
                                  dict(precision=PRECISION_FP32, rng=RNG_XOR128)],
                         ids=["fp32-mt19937", "fp64-xor128", "fp32-xor128"])
def test_modes(ren, mode):
    ren.set_scene(refscenes.ref4(), CAM)
    p = make_params(**REF4_13, **mode)
    with ren.film(p) as film:
        fill(film, film_ref.colours(refscenes.ref4(), CAM, p), [6, 7])
        against_one_shot(ren, film, p)


def test_final_scene_lds_bvh_lens_and_deferred_retries(ren):
    arr, cam = yk.build_scene("final", 42)
    ren.set_scene(arr, cam)
    p = make_params(32, 18, 13, 50, 404)
    with ren.film(p) as film:
        fill(film, film_ref.colours(arr, cam, p), [6, 7])
        against_one_shot(ren, film, p)


def test_mt_fallback(ren):
    arr, cam = yk.build_scene("glass", 42)
    ren.set_scene(arr, cam)
    p = make_params(16, 9, 8, 200, 404)
    with ren.film(p) as film:
        fill(film, film_ref.colours(arr, cam, p), [3, 5])
        against_one_shot(ren, film, p)


def test_seed_wrap(ren):
    ren.set_scene(refscenes.ref4(), CAM)
    p = make_params(48, 27, 4, 50, 4294967000)
    with ren.film(p) as film:
        fill(film, film_ref.colours(refscenes.ref4(), CAM, p), [1, 3])
        against_one_shot(ren, film, p)


@pytest.mark.parametrize("tile", [dict(rows=(1, 4, 2)), dict(cols=(3, 5, 1)), dict(rows=(1, 4, 2), cols=(3, 5, 1))],
                         ids=["rows", "cols", "rows-cols"])
def test_tiles(ren, tile):
    ren.set_scene(refscenes.ref4(), CAM)
    p = make_params(**REF4_13, **tile)
    with ren.film(p) as film:
        fill(film, film_ref.colours(refscenes.ref4(), CAM, p), [5, 8])
        against_one_shot(ren, film, p)


def test_a_film_and_other_renders_do_not_disturb_each_other(ren):
    ren.set_scene(refscenes.ref4(), CAM)
    p = make_params(**REF4_13)
    other = make_params(40, 22, 6, 50, 7, precision=PRECISION_FP32, rng=RNG_XOR128)
    other_alone = ren.render(other)
    cols = film_ref.colours(refscenes.ref4(), CAM, p)
    with ren.film(p) as film:
        between = []
        fill(film, cols, [5, 8], after=lambda done: between.append(ren.render(other)))
        assert all(same(b, other_alone) for b in between)
        against_one_shot(ren, film, p)


def test_two_films_on_one_context(ren):
    ren.set_scene(refscenes.ref4(), CAM)
    pa = make_params(**REF4_13)
    pb = make_params(24, 13, 9, 50, 99, rng=RNG_XOR128, rows=(2, 5, 2))
    ca, cb = film_ref.colours(refscenes.ref4(), CAM, pa), film_ref.colours(refscenes.ref4(), CAM, pb)
    (Sa, Qa), (Sb, Qb) = film_ref.prefixes(ca), film_ref.prefixes(cb)
    with ren.film(pa) as a, ren.film(pb) as b:
        for na, nb in ((5, 2), (1, 4), (7, 3)):
            a.accumulate(na)
            b.accumulate(nb)
            for film, S, Q in ((a, Sa, Qa), (b, Sb, Qb)):
                sums, sumsq, done = film.read()
                assert same(sums, S[done]) and same(sumsq, Q[done])
        against_one_shot(ren, a, pa)
        against_one_shot(ren, b, pb)


def test_set_scene_ends_a_film(ren):
    ren.set_scene(refscenes.ref4(), CAM)
    with ren.film(make_params(**REF4_13)) as film:
        film.accumulate(5)
        before = film.read()
        ren.set_scene(refscenes.ref4(), CAM)
        with pytest.raises(yk.YkError, match="YK_ERR_INVALID"):
            film.accumulate(8)
        after = film.read()  # the state it had stays readable
        assert same(before[0], after[0]) and same(before[1], after[1]) and after[2] == 5


def test_resume_from_a_saved_film(ren, tmp_path):
    ren.set_scene(refscenes.ref4(), CAM)
    p = make_params(**REF4_13)
    scene = yk.scene_hash(refscenes.ref4(), CAM)
    path = str(tmp_path / "film.ykfilm")
    with ren.film(p) as film:
        film.accumulate(5)
        film.save(path, scene)
    with ren.film(p) as film:
        assert film.done == 0
        assert film.load(path, scene) == 5
        S, Q = film_ref.prefixes(film_ref.colours(refscenes.ref4(), CAM, p))
        sums, sumsq, done = film.read()
        assert done == 5 and same(sums, S[5]) and same(sumsq, Q[5])
        film.accumulate(8)
        sums, sumsq, _ = film.read()
        assert same(sums, S[13]) and same(sumsq, Q[13])
        against_one_shot(ren, film, p)
    # another seed0, another target and another scene are refused, and change nothing
    for q in (make_params(**{**REF4_13, "seed0": 405}), make_params(**{**REF4_13, "spp": 14})):
        with ren.film(q) as film:
            with pytest.raises(yk.YkError, match="other render params"):
                film.load(path, scene)
            assert film.done == 0
    with ren.film(p) as film:
        with pytest.raises(yk.YkError, match="another scene"):
            film.load(path, yk.scene_hash(refscenes.lambert3(), CAM))
        assert film.done == 0


def test_random_device_key(ren):
    ren.set_scene(refscenes.ref4(), CAM)
    p = make_params(**REF4_13, seed_mode=SEED_RANDOM_DEVICE, seed_key=0x0123456789ABCDEF)
    with ren.film(p) as film:
        assert film.params.seed_key == 0x0123456789ABCDEF
        fill(film, film_ref.colours(refscenes.ref4(), CAM, p), [6, 7])
        against_one_shot(ren, film, p)
    # no key given: drawn once, at create, and the one every chunk renders with
    p0 = make_params(**REF4_13, seed_mode=SEED_RANDOM_DEVICE)
    with ren.film(p0) as film, ren.film(p0) as film2:
        key = film.params.seed_key
        assert key != 0 and film2.params.seed_key not in (0, key)
        for n in (6, 7):
            film.accumulate(n)
            assert ren.stats()["seed_key"] == key
        pk = make_params(**REF4_13, seed_mode=SEED_RANDOM_DEVICE, seed_key=key)
        against_one_shot(ren, film, pk)


def test_error_map(ren):
    ren.set_scene(refscenes.ref4(), CAM)
    p = make_params(**REF4_13)
    cols = film_ref.colours(refscenes.ref4(), CAM, p)
    S, Q = film_ref.prefixes(cols)
    with ren.film(p) as film:
        film.accumulate(1)
        with pytest.raises(yk.YkError, match="YK_ERR_INVALID"):
            film.error(0.0)
        for n in (1, 3, 8):  # done = 2, 5, 13
            done = film.accumulate(n)
            want = film_ref.e2_map(S[done], Q[done], done)
            thr = float(np.median(want))
            e2, st = film.error(thr)
            assert same(e2, want), f"e2 at {done}"
            over = int((want > thr).sum())
            assert 0 < over < want.size
            assert st == dict(pixels=want.size, pixels_over=over, max_e2=float(want.max()), samples_done=done,
                              samples_target=13)
            # without the map, and at the extremes of the threshold
            assert film.error(thr, want_map=False) == (None, st)
            assert film.error(float(want.max()))[1]["pixels_over"] == 0
            assert film.error(-1.0)[1]["pixels_over"] == want.size


def test_render_until(ren):
    ren.set_scene(refscenes.ref4(), CAM)
    p = make_params(**REF4_13)
    S, Q = film_ref.prefixes(film_ref.colours(refscenes.ref4(), CAM, p))
    maxima = {d: float(film_ref.e2_map(S[d], Q[d], d).max()) for d in (4, 8, 12, 13)}
    # a bound the image meets after 8 samples but not after 4 (if the maxima fall that way), else 13
    thr = np.sqrt(maxima[8])
    want = next((d for d in (4, 8, 12, 13) if maxima[d] <= thr * thr), 13)
    with ren.film(p) as film:
        st = film.render_until(thr, 4)
        assert st["samples_done"] == want == film.done
        assert (st["pixels_over"] == 0) == (maxima[want] <= thr * thr) and st["max_e2"] == maxima[want]
    with ren.film(p) as film:  # a bound nothing meets: the target ends it
        st = film.render_until(0.0, 4)
        assert st["samples_done"] == 13 and st["pixels_over"] > 0


def test_argument_errors(ren):
    ren.set_scene(refscenes.ref4(), CAM)
    lib = yk.load_library()
    p = make_params(**REF4_13)
    f = ctypes.c_void_p()
    assert lib.ykgpu_film_create(ren._ctx, None, ctypes.byref(f)) == 1
    assert lib.ykgpu_film_create(ren._ctx, ctypes.byref(p), None) == 1
    assert lib.ykgpu_film_accumulate(None, 1) == 1 and lib.ykgpu_film_resolve(None, None) == 1
    assert lib.ykgpu_film_read(None, None, None, None) == 1 and lib.ykgpu_film_error(None, 0.0, None, None) == 1
    assert lib.ykgpu_film_write(None, None, None, 0) == 1 and lib.ykgpu_film_params(None, None) == 1
    assert lib.ykgpu_film_destroy(None) == 0
    with pytest.raises(yk.YkError, match="YK_ERR_INVALID"):
        ren.film(make_params(16, 9, 0))
    with ren.film(p) as film:
        with pytest.raises(yk.YkError, match="YK_ERR_INVALID"):
            film.resolve()  # nothing accumulated
        film.accumulate(5)
        before = film.read()
        for n in (0, 9, 0xFFFFFFFF):
            with pytest.raises(yk.YkError, match="YK_ERR_INVALID"):
                film.accumulate(n)
        assert lib.ykgpu_film_resolve(film._f, None) == 1
        assert lib.ykgpu_film_write(film._f, None, before[1].ctypes.data, 5) == 1
        assert lib.ykgpu_film_write(film._f, before[0].ctypes.data, None, 5) == 1
        with pytest.raises(yk.YkError, match="YK_ERR_INVALID"):
            film.write(before[0], before[1], 14)
        after = film.read()
        assert same(before[0], after[0]) and same(before[1], after[1]) and after[2] == 5
        film.accumulate(8)  # exactly to the target
        against_one_shot(ren, film, p)


def cli(*args):
    return subprocess.run([yk.CLI_PATH, *args], capture_output=True, text=True, timeout=300)


COMMON = ("--width", "16", "--spp", "13", "--seed0", "404")


def test_cli_progressive_writes_the_plain_image(tmp_path):
    plain, prog = tmp_path / "plain.png", tmp_path / "prog.png"
    r = cli(*COMMON, str(plain))
    assert r.returncode == 0, r.stderr
    r = cli(*COMMON, "--progressive", "4", str(prog))
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines() == ["rendering...", "rendering finished", f"write to file : {prog}", "success"]
    assert prog.read_bytes() == plain.read_bytes()
    # --until: a bound nothing meets uses every sample and says so; a loose one stops early
    r = cli(*COMMON, "--progressive", "4", "--until", "0", str(prog))
    assert r.returncode == 0 and "samples used : 13" in r.stdout.splitlines()
    assert prog.read_bytes() == plain.read_bytes()
    r = cli(*COMMON, "--progressive", "4", "--until", "10", str(prog))
    assert r.returncode == 0 and "samples used : 4" in r.stdout.splitlines()


def test_cli_checkpoint_resumes_to_the_plain_image(tmp_path):
    plain, out, ck = tmp_path / "plain.png", tmp_path / "out.png", tmp_path / "film.ykfilm"
    assert cli(*COMMON, str(plain)).returncode == 0
    r = cli(*COMMON, "--progressive", "4", "--checkpoint", str(ck), "--stop-after", "1", str(out))
    assert r.returncode == 0, r.stderr
    assert "stopped at 4 of 13 samples" in r.stdout.splitlines()
    assert yk.load_film(str(ck))[2] == 4 and out.read_bytes() != plain.read_bytes()
    r = cli(*COMMON, "--progressive", "4", "--checkpoint", str(ck), str(out))
    assert r.returncode == 0, r.stderr
    assert yk.load_film(str(ck))[2] == 13 and out.read_bytes() == plain.read_bytes()
    # a checkpoint of other parameters or another scene is refused, and left as it is
    saved = ck.read_bytes()
    for other in (("--width", "16", "--spp", "13", "--seed0", "405"), (*COMMON, "--scene", "lambert3")):
        r = cli(*other, "--checkpoint", str(ck), str(tmp_path / "no.png"))
        assert r.returncode == 1 and r.stderr.startswith("raytrace: cannot resume: ")
        assert not (tmp_path / "no.png").exists() and ck.read_bytes() == saved
