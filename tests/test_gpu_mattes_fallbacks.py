"""The film mattes under the query kernels' forced stack: with the checked stack
limited to 2 entries (lib/abl/libykgpu_qstack2.so, the variant tests/test_gpu_fallbacks.py uses) the
matte kernel's lanes overflow it and take the ordered scan beside lanes that do not, and the table
must be the restatement's bytes all the same, as under the product library.  Each library runs in a
fresh child process (tests/mattes_child.py, selected by YKGPU_LIB_OVERRIDE)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import mattes_ref as mr
import uecraytracing_amd as yk
from uecraytracing_amd.records import make_params

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBS = {"product": "libykgpu.so", "qstack2": os.path.join("abl", "libykgpu_qstack2.so")}


def run_child(name, folder):
    lib = os.path.join(yk.LIB_DIR, LIBS[name])
    assert os.path.exists(lib), f"{lib}: built by uecraytracing_amd/csrc/Makefile (all)"
    env = dict(os.environ, YKGPU_LIB_OVERRIDE=lib)
    pr = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mattes_child.py"), str(folder)], env=env,
                        capture_output=True, text=True, timeout=240)
    assert pr.returncode == 0, pr.stderr[-2000:]
    with open(os.path.join(str(folder), "stats.json")) as f:
        stats = json.load(f)
    with np.load(os.path.join(str(folder), "out.npz")) as z:
        return {k: z[k] for k in z.files}, stats


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_mattes_under_the_forced_stack(tmp_path_factory):
    arr, cam = yk.read_scene(os.path.join(yk.SCENE_DIR, "final_seed42.yks"))
    want, wst = mr.table(arr, cam, make_params(32, 18, 8, 50, 404), 8)
    wc, wg, wcst = mr.coverage(want, [int(want["id"][9, 16, 0]), 0])
    for name in ("product", "qstack2"):
        got, st = run_child(name, tmp_path_factory.mktemp("mattes_" + name))
        assert same(got["table"], want), f"{name}: {int((got['table'] != want).sum())} of {want.size} pixels differ"
        assert {k: st["mattes"][k] for k in wst} == wst and st["mattes"]["redo_pixels"] == 0, name
        assert same(got["cov"], wc) and same(got["grey"], wg), name
        assert {k: st["coverage"][k] for k in wcst} == wcst, name
    assert 0 < wst["hits"] < wst["samples"]
