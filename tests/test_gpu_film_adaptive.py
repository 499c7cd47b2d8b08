"""Adaptive film passes on the MI355X (include/ykgpu.h "adaptive passes"): every pixel of a film
always holds exactly the first n_p terms of the one-shot render's fold.  Checked bit for bit, with
no tolerance, after every pass, against the numpy simulation of the selection rule on the oracle's
prefix folds (film_adaptive_ref).  The thresholds are quantiles of the reference's own error map,
so one pixel sits exactly on each and the strict `>` is exercised; what the reference selects in
each scenario is asserted as a precondition, so a degenerate input cannot pass silently.
"""
import subprocess

import numpy as np
import pytest

import film_adaptive_ref as far
import film_ref
import golden_data
import refscenes
import uecraytracing_amd as yk
from uecraytracing_amd.records import PRECISION_FP32, RNG_XOR128, make_params

pytestmark = pytest.mark.gpu

CAM = refscenes.reference_camera()
PASSES_A = far.PASSES_A
REF4_20 = dict(width=16, height=9, spp=20, max_depth=50, seed0=404)


@pytest.fixture(scope="module")
def ren():
    r = yk.Renderer(0)
    yield r
    r.close()


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check_state(film, sim, what):
    counts = film.counts()
    assert same(counts, sim.counts), f"counts {what}"
    sums, sumsq, done = film.read()
    assert done == int(sim.counts.min()) == film.done, f"done {what}"
    assert same(sums, sim.sums()), f"sums {what}"
    assert same(sumsq, sim.sumsq()), f"second moments {what}"
    assert film.count_range() == (int(sim.counts.min()), int(sim.counts.max()))
    if sim.counts.max() >= 1:
        assert same(film.resolve(), sim.image()), f"image {what}"
    if sim.counts.max() >= 2:
        want = sim.e2()
        thr = float(np.median(want[np.isfinite(want)]))
        e2, st = film.error(thr)
        assert same(e2, want), f"error map {what}"
        assert st == dict(pixels=want.size, pixels_over=int((want > thr).sum()), max_e2=float(want.max()),
                          samples_done=int(sim.counts.min()), samples_target=sim.target), f"error stats {what}"


def one_pass(ren, film, sim, q, n, what):
    thr2 = sim.threshold2(q)
    got = film.accumulate_adaptive(thr2, n).as_dict()
    want = sim.step(thr2, n)
    groups = want.pop("groups")
    want["groups"] = len(groups)
    print(what, "threshold2", thr2, "reference", want, groups, "film", got)
    assert got == want, what
    st = ren.stats()
    assert st["samples"] == want["samples_added"] and st["launches"] == want["launches"], what
    check_state(film, sim, what)
    return want, groups


def run(ren, spheres, cam, p, passes, selected=None, ngroups=None, last_groups=None):
    """Runs `passes` on a fresh film against the simulation; returns (film state, simulation)."""
    ren.set_scene(spheres, cam)
    sim = far.Sim(film_ref.colours(spheres, cam, p))
    seen = []
    with ren.film(p) as film:
        check_state(film, sim, "fresh")
        for i, (q, n) in enumerate(passes):
            want, groups = one_pass(ren, film, sim, q, n, f"after pass {i} {(q, n)}")
            seen.append((want["pixels_selected"], groups))
        # the preconditions: what the reference selects (the first pass is uniform)
        npix = sim.counts.size
        assert seen[0][0] == npix
        if selected is not None:
            assert [s for s, _ in seen[1:]] == selected, seen
        if ngroups is not None:
            assert [len(g) for _, g in seen[1:]] == ngroups, seen
        if last_groups is not None:
            assert seen[-1][1] == last_groups, seen
        state = film.read() + (film.counts(), film.resolve())
    return state, sim


def against_one_shot(ren, state, p):
    sums, _, done, counts, image = state
    assert done == p.samples_per_pixel and (counts == done).all()
    assert same(sums, ren.render_sums(p))
    assert same(image, ren.render(p))


def test_scenario_a_groups_launches_and_clamping(ren):
    p = make_params(**REF4_20)
    state, _ = run(ren, refscenes.ref4(), CAM, p, PASSES_A, selected=[36, 108, 68, 144], ngroups=[1, 2, 2, 5],
                   last_groups=[(4, 16), (7, 13), (11, 9), (12, 8), (16, 4)])
    assert far.launches_of(16) == 3 and far.launches_of(13) == 2 and far.launches_of(4) == 1  # (multi-launch groups)
    against_one_shot(ren, state, p)


@pytest.mark.parametrize("mode", [dict(precision=PRECISION_FP32), dict(rng=RNG_XOR128),
                                  dict(precision=PRECISION_FP32, rng=RNG_XOR128)],
                         ids=["fp32-mt19937", "fp64-xor128", "fp32-xor128"])
def test_modes(ren, mode):
    p = make_params(**REF4_20, **mode)
    state, sim = run(ren, refscenes.ref4(), CAM, p, PASSES_A)
    if len(mode) == 2:
        # the strict-comparison case: the 0.25-quantile threshold is exactly 0 and many pixels sit on it
        assert sim.threshold2(0.25) == 0.0 and int((sim.first_e2 == 0.0).sum()) == 55
    against_one_shot(ren, state, p)


def test_scenario_b_final_scene_lds_bvh_lens_and_deferred_retries(ren):
    arr, cam = yk.build_scene("final", 42)
    p = make_params(32, 18, 20, 50, 404)
    state, _ = run(ren, arr, cam, p, PASSES_A, selected=[144, 432, 228, 576])
    against_one_shot(ren, state, p)


def test_scenario_c_mt_fallback_and_a_take_of_one(ren):
    arr, cam = yk.build_scene("glass", 42)
    p = make_params(16, 9, 12, 200, 404)
    state, _ = run(ren, arr, cam, p, [(None, 3), (0.5, 4), (0.5, 4), (None, 12)], ngroups=[1, 1, 3],
                   last_groups=[(3, 9), (7, 5), (11, 1)])
    against_one_shot(ren, state, p)


def test_scenario_d_groups_smaller_than_a_block(ren):
    p = make_params(**REF4_20, rows=(1, 4, 2), cols=(3, 5, 1))
    state, sim = run(ren, refscenes.ref4(), CAM, p, PASSES_A, selected=[5, 15, 12, 20])
    assert sim.counts.size == 20
    against_one_shot(ren, state, p)


def test_scenario_e_whole_blocks_plus_a_rest_then_an_empty_pass(ren):
    p = make_params(24, 13, 10, 50, 404)
    ren.set_scene(refscenes.ref4(), CAM)
    sim = far.Sim(film_ref.colours(refscenes.ref4(), CAM, p))
    with ren.film(p) as film:
        picked = [one_pass(ren, film, sim, q, 3 if q else 4, f"pass {i}")[0]["pixels_selected"]
                  for i, q in enumerate((None, 0.5, 0.5))]
        assert picked == [312, 155, 137] and 155 == 2 * 64 + 27
        before = film.read() + (film.counts(),)
        got = film.accumulate_adaptive(sim.threshold2(0.5), 3).as_dict()  # selects nothing: YK_OK, no launch
        assert sim.step(sim.threshold2(0.5), 3)["pixels_selected"] == 0
        assert got == dict(pixels_selected=0, samples_added=0, groups=0, launches=0, min_count=4, max_count=10)
        st = ren.stats()
        assert st["launches"] == 0 and st["samples"] == 0
        after = film.read() + (film.counts(),)
        assert all(same(a, b) if isinstance(a, np.ndarray) else a == b for a, b in zip(before, after))
        check_state(film, sim, "after the empty pass")


def test_scenario_f_seed_wrap_in_compacted_groups(ren):
    p = make_params(48, 27, 6, 50, 4294967000)
    run(ren, refscenes.ref4(), CAM, p, [(None, 2), (0.5, 2), (0.5, 2)], selected=[648, 623])


def test_a_fresh_film_takes_a_uniform_chunk(ren):
    ren.set_scene(refscenes.ref4(), CAM)
    p = make_params(**REF4_20)
    with ren.film(p) as a, ren.film(p) as b:
        fp = a.accumulate_adaptive(-1.0, 13)
        assert fp.as_dict() == dict(pixels_selected=144, samples_added=144 * 13, groups=1, launches=2, min_count=13,
                                    max_count=13)
        assert b.accumulate(13) == 13
        sa, sb = a.read(), b.read()
        assert same(sa[0], sb[0]) and same(sa[1], sb[1]) and sa[2] == sb[2] == 13
        assert same(a.resolve(), b.resolve()) and same(a.error(0.0)[0], b.error(0.0)[0])
        assert a.accumulate(7) == 20  # uniform again: the plain call works on it
        against_one_shot(ren, a.read() + (a.counts(), a.resolve()), p)


def test_accumulate_on_a_non_uniform_film_is_refused(ren):
    ren.set_scene(refscenes.ref4(), CAM)
    p = make_params(**REF4_20)
    sim = far.Sim(film_ref.colours(refscenes.ref4(), CAM, p))
    with ren.film(p) as film:
        for i, (q, n) in enumerate(PASSES_A[:2]):
            one_pass(ren, film, sim, q, n, f"pass {i}")
        assert film.count_range() == (4, 9)
        with pytest.raises(yk.YkError, match="YK_ERR_INVALID.*ykgpu_film_accumulate_adaptive"):
            film.accumulate(1)
        with pytest.raises(yk.YkError, match="YK_ERR_INVALID"):
            film.accumulate_adaptive(0.0, 0)
        check_state(film, sim, "after the refused calls")
        assert film.done == 4 and film.read()[2] == 4
        # ykgpu_film_write makes it uniform again
        film.write(sim.S[5], sim.Q[5], 5)
        assert film.count_range() == (5, 5) and (film.counts() == 5).all()
        assert film.accumulate(15) == 20
        against_one_shot(ren, film.read() + (film.counts(), film.resolve()), p)


def test_a_film_and_other_renders_do_not_disturb_each_other(ren):
    ren.set_scene(refscenes.ref4(), CAM)
    p = make_params(**REF4_20)
    other = make_params(40, 22, 6, 50, 7, precision=PRECISION_FP32, rng=RNG_XOR128)
    other_alone = ren.render(other)
    sim = far.Sim(film_ref.colours(refscenes.ref4(), CAM, p))
    with ren.film(p) as film:
        for i, (q, n) in enumerate(PASSES_A):
            one_pass(ren, film, sim, q, n, f"pass {i}")
            assert same(ren.render(other), other_alone)
        against_one_shot(ren, film.read() + (film.counts(), film.resolve()), p)


def test_stale_scene(ren):
    ren.set_scene(refscenes.ref4(), CAM)
    with ren.film(make_params(**REF4_20)) as film:
        film.accumulate_adaptive(-1.0, 4)
        ren.set_scene(refscenes.ref4(), CAM)
        with pytest.raises(yk.YkError, match="YK_ERR_INVALID"):
            film.accumulate_adaptive(-1.0, 4)
        assert film.done == 4


def test_checkpoint_v2_resumes_to_the_uninterrupted_film(ren, tmp_path):
    ren.set_scene(refscenes.ref4(), CAM)
    p = make_params(**REF4_20)
    scene = yk.scene_hash(refscenes.ref4(), CAM)
    path = str(tmp_path / "film.ykfilm")
    whole, sim = run(ren, refscenes.ref4(), CAM, p, PASSES_A)
    part = far.Sim(film_ref.colours(refscenes.ref4(), CAM, p))
    with ren.film(p) as film:
        for i, (q, n) in enumerate(PASSES_A[:3]):
            one_pass(ren, film, part, q, n, f"pass {i}")
        film.save(path, scene)
    assert open(path, "rb").read(8) == b"ykfilm2\0"
    lp, lh, counts, sums, sumsq = yk.load_film_counts(path)
    assert bytes(lp) == bytes(p) and lh == scene and same(counts, part.counts)
    with ren.film(p) as film:
        film.write_counts(sums, sumsq, counts)
        check_state(film, part, "after write_counts")
        for i, (q, n) in enumerate(PASSES_A[3:]):
            one_pass(ren, film, part, q, n, f"resumed pass {3 + i}")
        got = film.read() + (film.counts(), film.resolve())
    assert all(same(a, b) if isinstance(a, np.ndarray) else a == b for a, b in zip(got, whole))
    with ren.film(p) as film:  # Film.load takes the same file
        assert film.load(path, scene) == 4
        assert same(film.counts(), counts)
        with pytest.raises(yk.YkError, match="YK_ERR_INVALID"):
            film.write_counts(sums, sumsq, np.full_like(counts, 21))
        assert same(film.counts(), counts)


def cli(*args):
    return subprocess.run([yk.CLI_PATH, *args], capture_output=True, text=True, timeout=300)


def test_cli_adaptive_and_its_checkpoint(tmp_path):
    p = make_params(**REF4_20)
    sim = far.Sim(film_ref.colours(refscenes.ref4(), CAM, p))
    sim.step(-1.0, 4)
    # the bound as the CLI reads it: a decimal string, squared there
    until = repr(float(np.sqrt(sim.threshold2(0.5))))
    thr2 = float(until) * float(until)
    passes = 1
    while sim.step(thr2, 4)["pixels_selected"]:
        passes += 1
    lo, hi, total = int(sim.counts.min()), int(sim.counts.max()), int(sim.counts.sum())
    assert passes > 2 and lo < hi  # (a proper adaptive run: some pixels stop early)
    common = ("--scene", "ref4", "--width", "16", "--spp", "20", "--seed0", "404", "--progressive", "4", "--until",
              until, "--adaptive")
    whole, out, ck = tmp_path / "whole.png", tmp_path / "out.png", tmp_path / "film.ykfilm"
    r = cli(*common, str(whole))
    assert r.returncode == 0, r.stderr
    assert f"samples used : {lo}..{hi} per pixel, {total} in all" in r.stdout.splitlines(), r.stdout
    rgb, W, H = golden_data.png_rgb(str(whole))
    assert (W, H) == (16, 9) and bytes(rgb) == sim.image().tobytes()
    # the same run in two parts through a v2 checkpoint
    r = cli(*common, "--checkpoint", str(ck), "--stop-after", "2", str(out))
    assert r.returncode == 0 and "stopped after 2 passes" in r.stdout.splitlines(), r.stdout + r.stderr
    assert ck.read_bytes()[:8] == b"ykfilm2\0" and out.read_bytes() != whole.read_bytes()
    r = cli(*common, "--checkpoint", str(ck), str(out))
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() == whole.read_bytes()
    assert same(yk.load_film_counts(str(ck))[2], sim.counts)
    # --adaptive without --until is rejected
    r = cli("--width", "16", "--spp", "20", "--adaptive", str(tmp_path / "no.png"))
    assert r.returncode == 2 and "adaptive" in r.stderr and not (tmp_path / "no.png").exists()
