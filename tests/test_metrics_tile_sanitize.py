"""CPU suite: the tile-fill geometry of the image metrics (csrc/firefly_tile.hpp at R = 5, section a4n) under AddressSanitizer and
UndefinedBehaviorSanitizer -- a stand-alone host program (tools/metrics_tile_sanitize.cpp), built and run here, never on a GPU.
Over images of 1..12 x 1..12 and 59..70 x 11..22, every tile: the 74 x 26 places of the luminance tile are each filled exactly once,
every slot flagged inside reads a table of exactly width * height texels, every in-image texel of a tile's footprint is read exactly
once, every pixel has exactly one owner; the eleven taps of a lane's fourteen rows stay inside the tile; and the flat indices of the
corner tiles of 16400 x 16400, 262149 x 1 and 1 x 70000 in size_t."""
import os
import subprocess

from conftest import ROOT


def test_metrics_tile_geometry_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "metrics_tile_sanitize"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", os.path.join(ROOT, "tools", "metrics_tile_sanitize.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=600)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    assert " 0 wrong" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stdout + r.stderr[-3000:]
    sizes = [(w, h) for h in range(1, 13) for w in range(1, 13)] + [(w, h) for h in range(11, 23) for w in range(59, 71)]
    fill = 74 * 26
    want = fill * (sum(-(-w // 64) * -(-h // 16) for w, h in sizes) + 3 * 4) + 4 * 64 * 14 * 11
    assert int(r.stdout.split()[1].rstrip(",")) == want, r.stdout
