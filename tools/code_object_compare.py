"""Kernel-by-kernel comparison of the gfx950 code of two builds of libmi_denoise.so (no GPU needed):

    python tools/code_object_compare.py --parent ../parent-checkout --change . [--out profiles/rNN_code_objects.txt]

Both arguments are source trees that have been built: the library is <tree>/image_denoising_filter_amd/libmi_denoise.so and the
names of its code objects, one per translation unit in link order, are the .hip files of SRCS in <tree>/Makefile.  Per translation
unit the table gives the code object's size and sha256 in both trees and the number of kernels compared and found identical.  A
kernel is identical when its function bytes (the symbol's .text range, _codeobj's section and symbol walk) and its 64-byte kernel
descriptor are the parent's; the descriptor's code-entry offset (bytes 16..23) is left out, it moves with the object's layout.
Whole code objects may differ in a few bytes outside the functions, so a unit whose hash moved is judged by its kernels.  Exit
status 1 when a kernel present in both trees differs, or when a tree has a kernel the other lacks that --gone / --new do not allow.
"""
import argparse
import hashlib
import os
import re
import sys

import importlib.util

# (the module alone: importing the package would load a library, and neither tree's need be the one next to this file)
_spec = importlib.util.spec_from_file_location(
    "_codeobj", os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "image_denoising_filter_amd", "_codeobj.py"))
_codeobj = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_codeobj)


def units(tree):
    """[(file name, code object bytes)] of a built tree."""
    mk = open(os.path.join(tree, "Makefile")).read()
    srcs = re.search(r"^SRCS\s*:=(.*?)(?<!\\)\n", mk, re.M | re.S).group(1)
    names = [os.path.basename(s) for s in srcs.replace("\\\n", " ").split() if s.endswith(".hip")]
    lib = os.path.join(tree, "image_denoising_filter_amd", "libmi_denoise.so")
    cos = _codeobj.gfx950_code_objects(open(lib, "rb").read())
    if len(cos) != len(names):
        raise SystemExit(f"{lib}: {len(cos)} code objects for {len(names)} .hip files of SRCS")
    return list(zip(names, cos)), lib


def kernels(co):
    """{mangled name: (function bytes, descriptor without its entry offset)} in symbol-value order."""
    syms = _codeobj._symbols(co)
    out = {}
    for name in sorted((n for n in syms if n + ".kd" in syms), key=lambda n: syms[n][1]):
        part = []
        for s, value, size in (syms[name], syms[name + ".kd"]):
            start = s["off"] + (value - s["addr"])
            part.append(co[start:start + size])
        out[name] = (part[0], part[1][:16] + part[1][24:])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--change", required=True)
    ap.add_argument("--out")
    ap.add_argument("--gone", default="", help="comma-separated .hip files whose kernels may disappear with the file")
    ap.add_argument("--new", default="", help="comma-separated .hip files that may appear with their kernels")
    args = ap.parse_args()
    (old, old_lib), (new, new_lib) = units(args.parent), units(args.change)
    new_by_name = dict(new)
    gone_ok = set(filter(None, args.gone.split(",")))
    new_ok = set(filter(None, args.new.split(",")))
    lines = ["gfx950 code objects of libmi_denoise.so, one per translation unit in link order (_codeobj.gfx950_code_objects): parent -> change",
             f"{'file':26s} {'parent bytes':>12s} {'sha256[:16]':16s} {'change bytes':>12s} {'sha256[:16]':16s}  kernels: compared / identical (function bytes, descriptor outside its entry offset)"]
    bad = []
    sha = lambda b: hashlib.sha256(b).hexdigest()[:16]
    for name, co in old:
        ko = kernels(co)
        if name not in new_by_name:
            lines.append(f"{name:26s} {len(co):12d} {sha(co):16s} {'-':>12s} {'-':16s}  removed with its {len(ko)} kernels")
            if name not in gone_ok:
                bad.append(f"{name} is gone")
            continue
        cn = new_by_name[name]
        kn = kernels(cn)
        both = [k for k in ko if k in kn]
        same = [k for k in both if ko[k] == kn[k]]
        order = "same order" if list(ko) == list(kn) else "ORDER OR SET DIFFERS"
        lines.append(f"{name:26s} {len(co):12d} {sha(co):16s} {len(cn):12d} {sha(cn):16s}  {len(both)} / {len(same)}, {order}"
                     + ("   whole object identical" if co == cn else ""))
        bad += [f"{name}: {k} differs" for k in both if k not in same]
        bad += [f"{name}: {k} only in the parent" for k in ko if k not in kn] + [f"{name}: {k} only in the change" for k in kn if k not in ko]
    for name, co in new:
        if name not in dict(old):
            lines.append(f"{name:26s} {'-':>12s} {'-':16s} {len(co):12d} {sha(co):16s}  new, {len(kernels(co))} kernels")
            if name not in new_ok:
                bad.append(f"{name} is new")
    for w in _codeobj.BENCH_KERNELS:
        a, b = (_codeobj.fingerprint(lib, w)["kernel_code_sha256"][:16] for lib in (old_lib, new_lib))
        lines.append(f"bench.py --workload {w}: timed kernel's code + descriptor sha256 {a} -> {b} {'identical' if a == b else 'DIFFERENT'}")
        if a != b:
            bad.append(f"fingerprint {w}")
    lines.append(f"library: {os.path.getsize(old_lib)} -> {os.path.getsize(new_lib)} bytes")
    lines.append(f"kernels that differ, appear or disappear outside the removed and the new files: {len(bad)}" + "".join("\n    " + b for b in bad))
    text = "\n".join(lines) + "\n"
    if args.out:
        open(args.out, "w").write(text)
    sys.stdout.write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
