"""CPU suite: the tile-fill geometry of the median filters (csrc/median_tile.hpp, section a4p) under AddressSanitizer and
UndefinedBehaviorSanitizer -- a stand-alone host program with its own main (tools/median_tile_sanitize.cpp), built and run here, never
on a GPU.  Over images from 1 x 1 to one past every seam, radius 1, 2, 3, every tile: every LDS slot is written once into a tile of
exactly the size the kernel allocates, every slot flagged inside reads a table of exactly width * height texels, every in-image texel of
a tile's footprint is read exactly once, a lane's window reads stay inside the tile, every pixel has exactly one owner; and the flat
indices of the corner tiles of 16400 x 16400, 262149 x 1 and 1 x 70000 in size_t."""
import os
import subprocess

from conftest import ROOT


def test_tile_fill_geometry_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "median_tile_sanitize"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", os.path.join(ROOT, "tools", "median_tile_sanitize.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=600)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    assert " 0 wrong" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stdout + r.stderr[-3000:]
    sizes = [(w, h) for h in range(1, 9) for w in range(1, 9)] + [(w, h) for h in (14, 15, 16, 17, 18, 30, 31, 32, 33, 34)
                                                                    for w in (62, 63, 64, 65, 66, 126, 127, 128, 129, 130)]
    want = 0
    for R in (1, 2, 3):
        fill = (64 + 2 * R) * (16 + 2 * R)
        want += fill * (sum(-(-w // 64) * -(-h // 16) for w, h in sizes) + 3 * 4)
    assert int(r.stdout.split()[1].rstrip(",")) == want, r.stdout
