"""The (radius, layer count) -> kernel class table of the joint bilateral, restated (opaque_vote_cases.joint_lds_bytes / joint_class)
and held against the three places that state it: csrc/bilateral_joint.hip, the sentence of include/mi_denoise.h (section a4e) and
the table of DESIGN.md 3.8.  tests/test_gpu_bilateral_joint_layers.py picks its cases on both sides of every boundary of this table
and asserts each case's class with the same function, so a changed tile shape moves this test and those cases together.
"""
import os
import re

import opaque_vote_cases as ov
from conftest import ROOT

LIMIT = 163840


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def tiled(r, L):
    return ov.joint_class(r, L, LIMIT) != "per pixel"


def test_the_restatement_is_the_sources():
    k = _read("image_denoising_filter_amd", "csrc", "bilateral_joint.hip")
    assert ov.JOINT_LDS_MAX == LIMIT
    assert re.search(r"return \(size_t\)\(64 \+ 2 \* radius\) \* \(tile_h \+ 2 \* radius\) \* \(sizeof\(float4\) \+ 3 \* sizeof\(float\) \* \(size_t\)n_layers\);", k)
    assert re.search(r"if \(n_layers > kJointTiledLayers\) return false;\s*if \(n_layers == 1\) return \(int\)bil_lds_bytes\(radius, tile_h, true\) <= lds_max;\s*"
                     r"return \(int\)joint_lds_bytes\(radius, tile_h, n_layers\) <= lds_max;", k)
    assert re.search(r"while \(l < kJointTiledLayers && joint_lds_bytes\(R, NW \* P, l \+ 1\) <= 160 \* 1024\) \+\+l;", k)
    assert re.search(r"if \(a\.n_layers > MAXL \|\| !joint_tiled\(ctx->lds_max, R, NW \* P, a\.n_layers\)\) return launch_generic\(a, R, s\);", k)
    assert re.search(r"if \(!joint_tiled\(ctx->lds_max, radius, kBilRtNW \* kBilRtP, a\.n_layers\)\) return launch_generic\(a, radius, s\);", k)
    assert re.search(r"sizeof\(float4\) \* \(split \? 2 : 1\);", _read("image_denoising_filter_amd", "csrc", "bilateral_shapes.hpp"))


def test_the_headers_sentence():
    h = " ".join(_read("include", "mi_denoise.h").replace("\n *", " ").split())
    assert "fit 160 KB -- T = 16 rows, 32 at radius 10, 8 at radius 20 -- which is every radius <= 8 at n_layers <= 4, radius <= 9 at 3, " \
           "radius <= 14 except 10 at 2; with one layer, the radii mid_bilateral_temporal's layered form runs tiled (<= 17 and 20)" in h
    assert {r: p * nw for r, (p, nw) in ov.BIL_SHAPES.items()} == {4: 16, 8: 16, 10: 32, 20: 8} and ov.BIL_RT_SHAPE[0] * ov.BIL_RT_SHAPE[1] == 16
    for r in range(1, 25):
        assert tiled(r, 4) == (r <= 8), r
        assert tiled(r, 3) == (r <= 9), r
        assert tiled(r, 2) == (r <= 14 and r != 10), r
        assert tiled(r, 1) == (r <= 17 or r == 20), r
        assert not any(tiled(r, L) for L in range(5, 17)), r
        for L in range(1, 5):
            assert ov.joint_class(r, L) in (("tuned", "per pixel") if r in ov.BIL_SHAPES else ("run-time radius", "per pixel"))
    # the cases test_gpu_bilateral_joint_layers.py runs: the largest tile per layer count, and the first radius past each boundary
    assert [ov.joint_lds_bytes(r, L) for r, L in ((14, 2), (9, 3), (7, 4), (8, 4))] == [161920, 144976, 149760, 163840]
    assert max(ov.joint_lds_bytes(r, L) for r in range(1, 25) for L in range(2, 5) if tiled(r, L) and r not in ov.BIL_SHAPES) == 161920
    for r, L in ((10, 2), (15, 2), (14, 3), (9, 4), (10, 3), (11, 3)):
        assert not tiled(r, L) and ov.joint_lds_bytes(r, L) > LIMIT, (r, L)


def test_designs_table():
    d = _read("DESIGN.md")
    assert "(64 + 2r)·(T + 2r)·(16 + 12·L) bytes, limit 163,840" in d
    rows = {m.group(1).strip(): m.group(0) for m in re.finditer(r"^\| ([^|]+) \|[^\n]*$", d[d.index("**(radius, L) → class**"):d.index("**Identities and parity**")], re.M)}

    def b(r, L):
        return f"{ov.joint_lds_bytes(r, L):,}"
    for r in (4, 8):
        assert [c.strip() for c in rows[str(r)].split("|")[3:8]] == [b(r, 1), b(r, 2), b(r, 3), b(r, 4), "per pixel"], r
        assert all(tiled(r, L) for L in (1, 2, 3, 4))
    assert [c.strip() for c in rows["10"].split("|")[3:5]] == [b(10, 1), f"per pixel ({b(10, 2)})"] and tiled(10, 1) and not tiled(10, 2)
    assert rows["20"].split("|")[3].strip() == b(20, 1) and rows["20"].count("per pixel") == 4 and tiled(20, 1) and not tiled(20, 2)
    others = [c.strip() for c in rows["1..9 others"].split("|")[3:8]]
    assert others == [f"≤ {b(9, 1)}", f"≤ {b(9, 2)}", f"≤ {b(9, 3)}", f"r ≤ 7: ≤ {b(7, 4)}; r = 9 per pixel ({b(9, 4)})", "per pixel"]
    assert all(tiled(r, L) for r in (1, 2, 3, 5, 6, 7, 9) for L in (1, 2, 3)) and all(tiled(r, 4) for r in (1, 2, 3, 5, 6, 7)) and not tiled(9, 4)
    assert [c.strip() for c in rows["11..14"].split("|")[3:6]] == [f"≤ {b(14, 1)}", f"≤ {b(14, 2)}", "per pixel"]
    assert all(tiled(r, L) for r in range(11, 15) for L in (1, 2)) and not any(tiled(r, 3) for r in range(11, 15))
    assert [c.strip() for c in rows["15..17"].split("|")[3:5]] == [f"≤ {b(17, 1)}", "per pixel"]
    assert all(tiled(r, 1) for r in range(15, 18)) and not any(tiled(r, 2) for r in range(15, 18))
    assert rows["18, 19, 21..24"].count("per pixel") == 5 and not any(tiled(r, L) for r in (18, 19, 21, 22, 23, 24) for L in (1, 2, 3, 4))
