"""CPU suite: the tap geometry of the recursive temporal accumulation (csrc/reproject_taps.hpp, section a4j) under AddressSanitizer
and UndefinedBehaviorSanitizer, float -> int conversions included -- a stand-alone host program (tools/reproject_taps_sanitize.cpp),
built and run here, never on a GPU.  It feeds the function the motion the GPU tests feed the kernel later (huge, infinite, NaN,
-0.0, the last float above -1) and reads a table of exactly width * height texels at every tap taken."""
import os
import subprocess

from conftest import ROOT


def test_tap_geometry_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "reproject_taps_sanitize"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", os.path.join(ROOT, "tools", "reproject_taps_sanitize.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=600)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    assert " 0 wrong" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stdout + r.stderr[-3000:]
    calls = int(r.stdout.split()[1])
    assert calls == 18 * 18 * sum(w * h for w in range(1, 6) for h in range(1, 6)), r.stdout
