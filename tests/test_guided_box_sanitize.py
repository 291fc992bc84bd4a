"""CPU suite: the geometry of the guided filter's sliding box sums (csrc/guided_box.hpp, section a4o) under AddressSanitizer and
UndefinedBehaviorSanitizer -- a stand-alone host program (tools/guided_box_sanitize.cpp), built and run here, never on a GPU.
Over images of 1..12 x 1..12 and the sizes around every wave, strip and restart seam, at radius 1, 2 and 16, every tile walked as the
kernels walk it: every pixel has exactly one owner, every prefix slot an output lane reads was filled in the same round, every global
index lies inside width * height, the rows inside a lane's running sum are exactly its window's and a segment's first output row
follows exactly 2 radius + 1 walked rows; and the corner tiles of 16400 x 16400, 262149 x 1 and 1 x 70000 in size_t."""
import os
import subprocess

from conftest import ROOT


def test_guided_box_geometry_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "guided_box_sanitize"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", os.path.join(ROOT, "tools", "guided_box_sanitize.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=600)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    assert " 0 wrong" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stdout + r.stderr[-3000:]
    assert int(r.stdout.split()[1]) > 10 ** 6, r.stdout
