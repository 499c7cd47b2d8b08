"""bench.py's command line and its --dump-outputs writer (CPU).

A plain run prints the headline figures only; the side measurements sit behind --full.
--dump-outputs writes the timed path's image as float32, whole when it fits the size limit, else
as a fixed, seeded sample that is the same from run to run."""
import sys

import numpy as np
import pytest

import bench


def parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_is_the_default(monkeypatch):
    a = parse(monkeypatch, "--gpus", "1", "--steps", "3", "--warmup", "2")
    assert (a.gpus, a.steps, a.warmup) == (1, 3, 2)
    assert a.full is False and a.dump_outputs is None
    a = parse(monkeypatch, "--full", "--dump-outputs", "somewhere")
    assert a.full is True and a.dump_outputs == "somewhere"


def test_steps_must_be_positive(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit, match="--steps"):
        bench.main()


def test_dump_outputs_writes_the_image_as_float32(tmp_path):
    torch = pytest.importorskip("torch")
    img = torch.arange(5 * 7 * 3, dtype=torch.int64).remainder(256).to(torch.uint8).reshape(5, 7, 3)
    bench.dump_outputs(str(tmp_path / "d"), img)
    got = np.load(tmp_path / "d" / "image.npy")
    assert got.dtype == np.float32 and got.shape == (5, 7, 3)
    np.testing.assert_array_equal(got, img.numpy().astype(np.float32))


def test_dump_outputs_samples_an_image_over_the_limit(tmp_path, monkeypatch):
    torch = pytest.importorskip("torch")
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4096)  # 1024 float32 values
    img = torch.arange(40 * 30 * 3, dtype=torch.int64).mul(7).remainder(256).to(torch.uint8).reshape(40, 30, 3)
    bench.dump_outputs(str(tmp_path / "a"), img)
    bench.dump_outputs(str(tmp_path / "b"), img)
    a, b = np.load(tmp_path / "a" / "image.npy"), np.load(tmp_path / "b" / "image.npy")
    assert a.dtype == np.float32 and a.shape == (512,) and a.nbytes <= 4096
    np.testing.assert_array_equal(a, b)
    # the sample is the image's bytes at the seeded positions, in image order
    idx = np.sort(np.random.default_rng(bench.DUMP_SAMPLE_SEED).choice(img.numel(), 512, replace=False))
    np.testing.assert_array_equal(a, img.numpy().reshape(-1)[idx].astype(np.float32))
