"""The plan of the NLM strip kernel's vertical patch sums (csrc/nlm_vbox_plan.hpp) on the host: no GPU.

tests/vbox_plan_host.cpp includes the header the kernels include and carries the planned additions out in float on small
integer-valued rows (every order exact) for patch widths 1..16, strips of 4 and 8 rows, the whole strip and both halves: every
output equals the box sum, a half performs exactly the whole strip's operations for its outputs (the bit-identity of the HALF
launch shape), 12 rows fold for the 7x7 patch at eight rows, and the fold counts match counts worked out by hand."""
import os
import subprocess

import pytest

from conftest import ROOT


@pytest.mark.parametrize("flags", [["-O1"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan_ubsan"])
def test_vbox_plan_host(tmp_path, flags):
    exe = tmp_path / "vbox_plan_host"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, os.path.join(ROOT, "tests", "vbox_plan_host.cpp"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "all checks passed" in r.stdout
