"""CPU suite: the tile-fill geometry of the firefly clamp (csrc/firefly_tile.hpp, section a4l) under AddressSanitizer and
UndefinedBehaviorSanitizer -- a stand-alone host program (tools/firefly_tile_sanitize.cpp), built and run here, never on a GPU.
Over images of 1..6 x 1..6 and 62..70 x 14..22, both radii, every tile: every slot flagged inside reads a table of exactly
width * height texels, every in-image texel of a tile's footprint is read exactly once, every pixel has exactly one owner; and the
flat indices of the corner tiles of 16400 x 16400 and 262149 x 2 in size_t."""
import os
import subprocess

from conftest import ROOT


def test_tile_fill_geometry_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "firefly_tile_sanitize"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", os.path.join(ROOT, "tools", "firefly_tile_sanitize.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=600)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    assert " 0 wrong" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stdout + r.stderr[-3000:]
    sizes = [(w, h) for h in range(1, 7) for w in range(1, 7)] + [(w, h) for h in range(14, 23) for w in range(62, 71)]
    want = 0
    for R in (1, 2):
        fill = (64 + 2 * R) * (16 + 2 * R)
        want += fill * (sum(-(-w // 64) * -(-h // 16) for w, h in sizes) + 2 * 4)
    assert int(r.stdout.split()[1].rstrip(",")) == want, r.stdout
