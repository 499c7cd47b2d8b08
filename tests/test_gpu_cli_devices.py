"""raytrace --devices: every film option through a group film (include/ykgpu.h "group films").  The
same command with and without --devices 0,0,0 writes the same bytes: the image, the feature PNGs and
the checkpoint's arrays.  The list's grammar is the bridge's device list (YKGPU_DEVICES)."""
import subprocess

import numpy as np
import pytest

import uecraytracing_amd as yk


def cli(*args):
    return subprocess.run([yk.CLI_PATH, *args], capture_output=True, text=True, timeout=300)


def test_a_bad_device_list_is_reported(tmp_path):
    out = str(tmp_path / "o.png")
    r = cli("--devices", "0,x", out)
    assert r.returncode != 0 and "--devices: not a device list" in r.stderr
    r = cli("--devices", "0,", out)
    assert r.returncode != 0 and "--devices" in r.stderr
    r = cli("--devices", "0", "--device", "0", out)
    assert r.returncode == 2 and "exclude each other" in r.stderr


@pytest.mark.gpu
def test_every_film_option_over_three_entries_equals_one_device(tmp_path):
    common = ("--scene", "mixed12", "--width", "96", "--spp", "16", "--seed0", "404", "--progressive", "4",
              "--until", "0.02", "--adaptive", "--denoise-features")
    runs = {}
    for name, extra in (("one", ()), ("three", ("--devices", "0,0,0"))):
        d = tmp_path / name
        d.mkdir()
        r = cli(*common, *extra, "--checkpoint", str(d / "film.ykfilm"), "--aov", str(d / "f"), str(d / "o.png"))
        assert r.returncode == 0, r.stderr
        runs[name] = (d, r.stdout.replace(str(d), "DIR"))
    (a, out_a), (b, out_b) = runs["one"], runs["three"]
    assert out_a == out_b and "samples used : " in out_a  # the same passes, the same samples per pixel
    for png in ("o.png", "f.albedo.png", "f.normal.png", "f.depth.png"):
        assert (a / png).read_bytes() == (b / png).read_bytes(), png
    pa, ha, ca, sa, qa = yk.load_film_counts(str(a / "film.ykfilm"))
    pb, hb, cb, sb, qb = yk.load_film_counts(str(b / "film.ykfilm"))
    assert bytes(pa) == bytes(pb) and ha == hb
    assert ca.tobytes() == cb.tobytes() and sa.tobytes() == sb.tobytes() and qa.tobytes() == qb.tobytes()
    assert ca.shape == (54, 96) and ca.min() >= 4 and ca.min() != ca.max()  # (an adaptive run: counts differ)
    # the checkpoint of the group run resumes on one device, and the other way round: nothing left to do
    for d, extra in ((b, ()), (a, ("--devices", "0,0"))):
        before = (d / "o.png").read_bytes()
        r = cli(*common, *extra, "--checkpoint", str(d / "film.ykfilm"), str(d / "o.png"))
        assert r.returncode == 0, r.stderr
        assert (d / "o.png").read_bytes() == before
