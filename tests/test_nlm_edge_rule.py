"""The packed right-edge shape of the NLM strip kernel (csrc/nlm_edge.hip, nlm_strip.hpp TAG = kNlmEdgeTag), host side: the rule that decides
which frames pack, restated here and held against the constants and the text of the sources.

The rule.  A wave yields VW = 64 - (PW - 1) columns; the last tile column of a frame holds valid = w - (tiles_x - 1) * VW of the image's.
Packed, a wave is four groups of 16 lanes, one tile each; a valid lane's horizontal sum reaches PW - 1 lanes beyond the valid ones, all of
which must be REAL columns of the group: valid + PW - 1 <= 12.  A real column reads its search range, SW texels of a tile row, so
12 + SW - 1 <= 32, the pitch; the tall tile is 32 x (4 * 32 + PW - 1 + SW - 1) texels of 16 bytes and must leave room for two workgroups
a CU (<= 80 KB of the 160).
"""
import os
import re

import opaque_vote_cases as ov
from conftest import ROOT

CSRC = os.path.join(ROOT, "image_denoising_filter_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def constants():
    m = re.search(r"constexpr int kNlmEdgeTag = (\d+), kNlmEdgeGroups = (\d+), kNlmEdgeLanes = (\d+), kNlmEdgeCols = (\d+), kNlmEdgePitch = (\d+);",
                  _src("nlm_strip.hpp"))
    assert m, "the packed shape's constants"
    return dict(zip(("tag", "groups", "lanes", "cols", "pitch"), map(int, m.groups())))


def valid_columns(w, patch_w):
    vw = 64 - (patch_w - 1)
    return w - (-(-w // vw) - 1) * vw


def packs(w, patch_w):
    return -(-w // (64 - (patch_w - 1))) >= 2 and valid_columns(w, patch_w) + patch_w - 1 <= 12


def test_the_constants_are_the_rules():
    c = constants()
    assert c == dict(tag=2, groups=4, lanes=16, cols=12, pitch=32)
    assert c["groups"] * c["lanes"] == 64 and c["cols"] <= c["lanes"]
    for name, (search, patch) in ov.NLM_WINDOWS.items():
        sw, pw = search[1] - search[0], patch[1] - patch[0]
        r, nw = ov.NLM_STRIP_SHAPES["whole"]
        assert c["cols"] + sw - 1 <= c["pitch"], name                  # a real column's search range stays in its tile row
        rows = c["groups"] * r * nw + pw - 1 + sw - 1
        lds = c["pitch"] * rows * 16
        assert lds <= 80 * 1024, (name, lds)                           # two workgroups a CU
        assert lds == {"bench": 78848, "ref": 74752}[name]
        most = c["cols"] - (pw - 1)                                    # the most valid columns that pack
        assert most == {"bench": 6, "ref": 7}[name]
        nl, nr = -patch[0], patch[1] - 1
        assert nl + most + nr <= c["cols"] and nl + most - 1 <= c["lanes"] - 1 - nr   # every lane a valid lane's sum reaches is a real column of its group
        # a clamped lane (from `cols` on) still reads inside the row: column min(col, pitch - SW) + SW - 1 <= pitch - 1
        assert max(min(col, c["pitch"] - sw) + sw - 1 for col in range(c["lanes"])) <= c["pitch"] - 1
        assert all(min(col, c["pitch"] - sw) == col for col in range(c["cols"])), "no real column is clamped"


def test_which_frames_pack():
    assert valid_columns(1920, 7) == 6 and packs(1920, 7)              # 1920 = 33 x 58 + 6
    assert valid_columns(1280, 7) == 4 and packs(1280, 7)              # 1280 = 22 x 58 + 4
    assert valid_columns(122, 7) == 6 and packs(122, 7) and valid_columns(124, 7) == 8 and not packs(124, 7)
    assert valid_columns(116, 7) == 58 and not packs(116, 7)           # no ragged column
    assert valid_columns(6, 7) == 6 and not packs(6, 7)                # a single tile column is the main launch's
    assert [w for w in range(59, 59 + 58) if packs(w, 7)] == list(range(59, 65))
    assert [w for w in range(60, 60 + 59) if packs(w, 6)] == list(range(60, 67))
    # the benchmark's launch: 31 frames of 1920 x 1080
    tiles_x, tiles_y = -(-1920 // 58), -(-1080 // 32)
    assert ov.nlm_tile_workgroups(1920, 1080, 7, 31) == 35836
    assert (tiles_x - 1) * tiles_y * 31 == 34782 and -(-tiles_y // 4) * 31 == 279


def test_the_sources_state_the_rule():
    strip, edge, nlm = _src("nlm_strip.hpp"), _src("nlm_edge.hip"), _src("nlm.hip")
    assert re.search(r"constexpr int nlm_edge_valid\(int w, int patch_w\) \{ return w - \(w - 1\) / \(64 - \(patch_w - 1\)\) \* \(64 - \(patch_w - 1\)\); \}", strip)
    assert re.search(r"constexpr bool nlm_edge_packs\(int valid, int patch_w, int tiles_x\) \{ return tiles_x >= 2 && valid \+ patch_w - 1 <= kNlmEdgeCols; \}", strip)
    assert re.search(r"constexpr int nlm_edge_tile_rows\(int tile_h, int patch_w, int search_w\) \{ return kNlmEdgeGroups \* tile_h \+ patch_w - 1 \+ search_w - 1; \}", strip)
    for w in range(1, 400):                                            # (w - 1) / VW == tiles_x - 1
        for pw in (6, 7):
            vw = 64 - (pw - 1)
            assert w - (w - 1) // vw * vw == valid_columns(w, pw)
    assert re.search(r"constexpr bool EDGE = TAG == kNlmEdgeTag;", strip) and re.search(r"constexpr bool kOpaqueForm = !RTS && !EDGE;", strip)
    assert re.search(r"col < kNlmEdgePitch - SW \? col : kNlmEdgePitch - SW", strip)
    assert re.search(r"static_assert\(lds_bytes <= 80 \* 1024", edge)
    assert re.search(r"nlm_strip_kernel<SLO, SHI, PLO, PHI, 8, 4, FMT, FUSED, false, false, kNlmEdgeTag>", edge)
    windows = {tuple(map(int, m)) for m in re.findall(r"edge_window<(-?\d+), (-?\d+), (-?\d+), (-?\d+)>", edge)}
    assert windows == {s + p for s, p in ov.NLM_WINDOWS.values()}
    for fmt in ("RGBA8", "RGBA16F", "RGBA32F"):
        for fused in ("true", "false"):
            assert f"launch_edge<SLO, SHI, PLO, PHI, MID_FMT_{fmt}, {fused}>" in edge
    # packed: k = 0, not a launch of the frame pipeline, not while the stream records; the main launch leaves the column out
    assert re.search(r"a\.k == 0 && !a\.corunning &&\s*nlm_edge_packs\(nlm_edge_valid\(a\.w, pw\), pw, [^;]*\) && !stream_is_recording\(s\);", edge)
    assert re.search(r"int rc = main_launch\(ctx, a, s, 1\);", edge) and len(re.findall(r"return main_launch\(ctx, a, s, 0\);", edge)) == 2
    assert len(re.findall(r"return nlm_dispatch_edge\(ctx, p, a, s, FMT, FUSED,", nlm)) == 2
    assert re.search(r"a\.tiles_x = \(int\)cdiv\(a\.w, VW\) - less_cols;", strip)
    with open(os.path.join(ROOT, "Makefile")) as f:
        mk = f.read()
    assert "$(CSRC)/nlm_edge.hip" in mk and re.search(r"^EXTRA_nlm_edge\.hip := \$\(EXTRA_nlm\.hip\)$", mk, re.M), "compiled with nlm.hip's flags"
