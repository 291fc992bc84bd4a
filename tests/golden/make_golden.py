"""Regenerates tests/golden/*.npz.  Run from the repo root IN THE BUILD CONTAINER
(needs /root/reference for the _ref part):   python tests/golden/make_golden.py

Two kinds of fixture, kept apart by file name:
  ref_cpu_bilateral_*.npz  inputs + outputs of the REFERENCE's own CPU loop
                           (src/main.cpp:1827-1864 compiled by oracle/Makefile into oracle/_ref).
                           These pin oracle.c::orc_cpu_bilateral and anything checked against it.
  shader_*.npz             inputs + outputs of oracle.c's shader restatements (a1-a5).  The
                           reference offers nothing to pin these ("parity unpinned"): they only
                           freeze the restatement so that an accidental edit of oracle.c, or a
                           compiler/libm change, is detected.
A fixture is data (seeded inputs, expected outputs); no reference source text is stored.

shard_plans.json is not rewritten by the run above: see save_shard_plans.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle  # noqa: E402
from conftest import synth_hdr, synth_ldr  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))


def save(name, **arrays):
    """np.savez_compressed, but an existing fixture with identical content is left alone (zip members carry
    timestamps, so rewriting would change the file's bytes for nothing)."""
    path = os.path.join(OUT, name)
    if os.path.exists(path):
        old = np.load(path)
        if sorted(old.files) == sorted(arrays) and all(np.array_equal(old[k], np.asarray(v)) for k, v in arrays.items()):
            return
    np.savez_compressed(path, **arrays)
    if os.path.getsize(path) > 1 << 20:
        save_compact(path, arrays)


def save_compact(path, arrays):
    """The same .npz (np.load reads it as usual and returns equal arrays) for a fixture that deflate leaves above the 1 MiB a
    committed file may have: LZMA members, and 8-bit images stored channel by channel (Fortran order), which compresses better."""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w") as zf:
        for k, v in arrays.items():
            v = np.asarray(v)
            b = io.BytesIO()
            np.lib.format.write_array(b, np.asfortranarray(v) if v.dtype == np.uint8 and v.ndim == 3 else v, allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), b.getvalue(), compress_type=zipfile.ZIP_LZMA)


def main():
    oracle.build()
    if not oracle.have_ref():
        raise SystemExit("oracle/_ref is missing: run in the container that has /root/reference")
    rng = np.random.default_rng(20250205)

    # --- the reference's own loop ------------------------------------------------------------
    for name, (h, w, R), kind in (("a", (40, 48, 10), "hdr"), ("b", (29, 37, 4), "ldr"), ("c", (24, 31, 10), "rand")):
        if kind == "hdr":
            img = synth_hdr(rng, h, w, 2.0)
        elif kind == "ldr":
            img = oracle.unpack_u8(synth_ldr(rng, h, w), flavour=1)
        else:
            img = rng.random((h, w, 4), dtype=np.float32)
        out1 = oracle.ref_cpu_bilateral(img, R, threads=1)
        out8 = oracle.ref_cpu_bilateral(img, R, threads=8)
        assert np.array_equal(out1, out8)
        save(f"ref_cpu_bilateral_{name}.npz", img=img, radius=R, out=out1)

    # --- the reference's loop on BLUE-CONSTANT images ------------------------------------------
    # With blue constant the loop's typo `texColor.b - texColor.b` (src/main.cpp:1850) is also the true
    # blue difference, so the loop IS the shaders' bilateral formula (sigma_s=10, sigma_c=0.2) on the
    # interior -- its output can be held directly against the GPU kernels (a1, a2, a3), no oracle between.
    rb = np.random.default_rng(20251004)
    for name, (h, w, R), kind in (("d", (64, 80, 10), "hdr"), ("e", (64, 80, 4), "ldr"), ("f", (45, 53, 10), "hdr"),
                                  ("g", (45, 53, 4), "ldr")):
        if kind == "hdr":
            img = synth_hdr(rb, h, w, 2.0)
            img[..., 2] = 0.375
            u8 = np.zeros((0,), np.uint8)
        else:
            u8 = synth_ldr(rb, h, w)
            u8[..., 2] = 96                                  # constant blue code, alpha is 255 already
            img = oracle.unpack_u8(u8, flavour=1)            # the CPU path's decode, src/main.cpp:1804-1807
        out1 = oracle.ref_cpu_bilateral(img, R, threads=1)
        assert np.array_equal(out1, oracle.ref_cpu_bilateral(img, R, threads=8))
        save(f"ref_blue_const_{name}.npz", img=img, img_u8=u8, radius=R, out=out1)

    # --- the cases tests/test_oracle.py runs against the loop itself where oracle/_ref is built -------------
    # (same seeds and shapes as there): the loop's output at -O2 and at the reference's own flags, so that the
    # tests hold the oracle against the reference everywhere else too
    cases = {}
    for (h, w), R in (((33, 41), 10), ((21, 25), 10), ((30, 19), 4), ((64, 64), 7)):
        img = np.random.default_rng(R * 100 + h).random((h, w, 4), dtype=np.float32) * 1.5
        cases[f"img_{h}x{w}_r{R}"] = img
        cases[f"out_{h}x{w}_r{R}"] = oracle.ref_cpu_bilateral(img, R, 2)
    img = np.random.default_rng(9).random((37, 53, 4), dtype=np.float32) * 2.0
    cases["as_shipped_img"] = img
    for R, th in ((10, 1), (4, 3)):
        cases[f"as_shipped_O2_r{R}_t{th}"] = oracle.ref_cpu_bilateral(img, R, th)
        cases[f"as_shipped_O0_r{R}_t{th}"] = oracle.ref_cpu_bilateral(img, R, th, as_shipped=True)
    save("ref_cpu_bilateral_cases.npz", **cases)

    # --- BASELINE configs[0]: 512x512 8-bit PNG, CPU bilateral r=4 ------------------------------
    # Input as the reference decodes a PNG for the CPU path (c * (1/255), :1804-1807), the loop's float output
    # (kept as a SHA-256 of its bits plus every 32nd row -- 4 MB of floats is not a small fixture) and the PNG
    # the reference would write: the truncating pack of :1905-1911 applied to the loop's output.
    import hashlib
    rc = np.random.default_rng(1)                            # seed 1
    u8 = synth_ldr(rc, 512, 512)
    out = oracle.ref_cpu_bilateral(oracle.unpack_u8(u8, flavour=1), 4, threads=8)
    save("ref_cpu_config0_512.npz", img_u8=u8, radius=4, out_u8=oracle.pack_u8(out), out_rows=out[::32],
         out_sha256=np.frombuffer(hashlib.sha256(out.tobytes()).digest(), np.uint8))

    # --- shader restatements (unpinned; regression only) -------------------------------------
    h, w = 29, 37
    hdr = synth_hdr(rng, h, w, 3.0)
    ldr = synth_ldr(rng, h, w)
    layers = [synth_ldr(rng, h, w) for _ in range(2)]
    nb = (hdr * rng.gamma(16.0, 1 / 16.0, (h, w, 1))).astype(np.float32)
    W0 = np.zeros((h, w, 8), np.float32)
    fix = dict(hdr=hdr, ldr=ldr, layer0=layers[0], layer1=layers[1], nb=nb)
    fix["bil_tex_r4"] = oracle.bilateral_texture(hdr, 4, 2.0, 0.2)
    fix["bil_lin_r4"] = oracle.bilateral_linear(hdr, 4, 2.0, 0.2)
    fix["bil_tex_r8_ldr"] = oracle.bilateral_texture(oracle.unpack_u8(ldr, 0), 8, 2.0, 0.2)
    Wl = oracle.bilateral_layers_accum(hdr, layers[0], W0, 4, 2.0, 0.2)
    Wl = oracle.bilateral_layers_accum(hdr, layers[1], Wl, 4, 2.0, 0.2)
    fix["layers_W"] = Wl
    fix["layers_out"] = oracle.normalize(Wl)
    hs = (hdr * 0.25).astype(np.float32)
    ns = (nb * 0.25).astype(np.float32)
    fix["nlm_in_t"], fix["nlm_in_n"] = hs, ns
    Wn = oracle.nlm_accum(hs, ns, W0, 0.5, (-7, 7), (-3, 3))
    fix["nlm_ref_W"] = Wn
    fix["nlm_bench_W"] = oracle.nlm_accum(hs, ns, W0, 0.5, (-10, 11), (-3, 4))
    fix["nlm_ref_out"] = oracle.normalize(Wn)
    save("shader_restatement.npz", **fix)
    print("wrote", sorted(os.listdir(OUT)))


def save_shard_plans():
    """tests/golden/shard_plans.json: a PINNED RECORD of the frame-block shard plan (csrc/sharded.cpp, through the wrappers of
    image_denoising_filter_amd/sharding.py) for every (n, world, k, rank) of tests/test_shard_native_plan.py's CASES, one row
    per line: [n, world, k, rank, partition(n, world), halo_plan(n, world, k, rank), block_launch_plan(n, world, k, rank)].
    First written while an independent Python statement of the plan still agreed with the C++ one.  Regenerate it only on a
    DELIBERATE plan change, never to make a failing test pass:   python tests/golden/make_golden.py shard_plans"""
    import json
    from image_denoising_filter_amd import sharding
    from test_shard_native_plan import CASES
    rows = [[n, world, k, rank, sharding.partition(n, world), sharding.halo_plan(n, world, k, rank),
             sharding.block_launch_plan(n, world, k, rank)] for n, world, k in CASES for rank in range(world)]
    with open(os.path.join(OUT, "shard_plans.json"), "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in rows) + "\n]\n")


if __name__ == "__main__":
    if sys.argv[1:] == ["shard_plans"]:
        save_shard_plans()
    else:
        main()
