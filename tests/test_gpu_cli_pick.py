"""raytrace --pick on the MI355X: the line it prints for a pixel carries the yardstick's values
(cast_ref on the pixel-centre pinhole ray, %.17g: every double round-trips) for a hit pixel and for a
sky pixel of the ref4 scene, and no image is rendered.  (The argument errors need no device:
test_cast_ref.py.)"""
import subprocess

import pytest

import cast_ref
import refscenes
import uecraytracing_amd as yk
from uecraytracing_amd import records

pytestmark = pytest.mark.gpu

CAM = refscenes.reference_camera()
W, H = 64, 36


def cli(*args):
    return subprocess.run([yk.CLI_PATH, *args], capture_output=True, text=True, timeout=300)


def expected(x, y):
    o, d = cast_ref.pixel_rays(CAM, W, H)
    r = cast_ref.cast(refscenes.ref4(), o[y * W + x], d[y * W + x], records.T_MIN, float("inf"))[0]
    if not r["flags"] & records.HIT_HIT:
        return f"pick {x} {y}: miss"
    v = lambda a: "(" + ", ".join("%.17g" % c for c in a) + ")"
    front = 1 if r["flags"] & records.HIT_FRONT_FACE else 0
    return f"pick {x} {y}: id {r['id']} t {'%.17g' % r['t']} p {v(r['p'])} normal {v(r['normal'])} front {front}"


@pytest.mark.parametrize("x,y,kind", [(32, 18, "id 0 "), (10, 17, "id 2 "), (40, 33, "id 1 "), (0, 0, "miss"), (63, 2, "miss")])
def test_pick_prints_the_yardsticks_record(tmp_path, x, y, kind):
    want = expected(x, y)
    assert kind in want, want
    r = cli("--scene", "ref4", "--width", str(W), "--pick", f"{x},{y}")
    assert r.returncode == 0, r.stderr
    assert r.stdout == want + "\n"
    assert "rendering" not in r.stdout and not list(tmp_path.iterdir())
    # an output file on the command line is not written either
    out = tmp_path / "o.png"
    r = cli("--scene", "ref4", "--width", str(W), f"--pick={x},{y}", str(out))
    assert r.returncode == 0 and r.stdout == want + "\n" and not out.exists()
