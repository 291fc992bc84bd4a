"""Per-kernel static figures of device code, for two source trees side by side (no GPU needed):

    python tools/kernel_static_table.py --parent ../parent-checkout --change . [--out profiles/rNN_static.txt]
                                        [--trailing-defaults "1, true"] [file.hip ...]

Each file (default: the four layer-filter files) is compiled to gfx950 assembly with the Makefile's flags for that file, in both
trees; per kernel the table gives vgpr_count, sgpr_count, private_segment_fixed_size (scratch), group_segment_fixed_size (static
LDS) and the number of v_exp_f32 / ds_read_b128 / ds_read_b96 in its body, parent -> change where they differ.  The closing lines
say whether any kernel gained scratch or static LDS, fell into a lower waves-per-SIMD class (512 VGPRs per lane and SIMD,
allocated in granules of 8, at most 8 waves), or traded a ds_read_b128 for a ds_read_b96.

--trailing-defaults ARGS: the change added template arguments with default values at the END of some kernels' argument lists.  A
kernel of the change whose demangled name ends in ", ARGS>" (several ARGS may be given, separated by ";") is compared with the
parent's kernel of the same name without them; the change's other new instantiations are listed with their own figures.  The
last column says whether a kernel's instructions are the parent's, text for text (its own name aside).
"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

FILES = ["bilateral.hip", "bilateral_temporal.hip", "nlm_layers.hip", "nlm_layers_temporal.hip"]
COUNTED = ("v_exp_f32", "ds_read_b128", "ds_read_b96")
META = ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")


def flags(tree, name):
    """HIPFLAGS and EXTRA_<file> of the tree's Makefile, its variables expanded."""
    text = open(os.path.join(tree, "Makefile")).read()
    var = {k: v.strip() for k, v in re.findall(r"^(\w[\w.]*)\s*[:?]?=\s*(.*)$", text, re.M)}

    def expand(v, depth=0):
        return v if depth > 4 else re.sub(r"\$\((\w[\w.]*)\)", lambda m: expand(var.get(m.group(1), ""), depth + 1), v)
    return expand(var["HIPFLAGS"]).split() + expand(var.get("EXTRA_" + name, "")).split()


def assembly(tree, name, hipcc):
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, name + ".s")
        src = os.path.join("image_denoising_filter_amd", "csrc", name)
        subprocess.run([hipcc, *flags(tree, name), "--cuda-device-only", "-S", src, "-o", out], check=True, cwd=tree)
        return open(out).read()


def kernels(asm):
    """{mangled name: {figure: value}} of one assembly listing."""
    table = {}
    for m in re.finditer(r"^\s*- \.agpr_count:.*?(?=^\s*- \.agpr_count:|^amdhsa\.target|\Z)", asm, re.M | re.S):
        block = m.group(0)
        name = re.search(r"^\s*\.name:\s*(\S+)", block, re.M).group(1)
        table[name] = {k: int(re.search(rf"^\s*\.{k}:\s*(\d+)", block, re.M).group(1)) for k in META}
    for name, row in table.items():
        start = re.search(rf"^{re.escape(name)}:", asm, re.M).end()
        body = asm[start:asm.index(".amdhsa_kernel " + name, start)]
        for ins in COUNTED:
            row[ins] = len(re.findall(rf"^\s*{ins}(?:_e32|_e64)?\b", body, re.M))
        # the instructions alone: no comments, labels or directives, and neither the kernel's own name nor its number in the file
        row["text"] = "\n".join(ln.split(";")[0].strip() for ln in re.sub(r"\.LBB\d+_", ".LBB_", body.replace(name, "K")).splitlines()
                                if ln.startswith("\t") and not ln.lstrip().startswith((".", ";")))
    return table


def waves(vgprs):
    return min(8, 512 // max(8, (vgprs + 7) // 8 * 8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--change", required=True)
    ap.add_argument("--out")
    ap.add_argument("--hipcc", default=os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    ap.add_argument("--trailing-defaults", default="")
    ap.add_argument("files", nargs="*", default=FILES)
    args = ap.parse_args()
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")      # (without one the table shows the mangled names)
    lines, verdict = [], {"scratch": [], "lds": [], "waves": [], "b96": [], "missing": []}
    trailing = [t.strip() for t in args.trailing_defaults.split(";") if t.strip()]
    demangle = lambda names: dict(zip(names, subprocess.run([filt, *names], capture_output=True, text=True).stdout.splitlines())) if filt and names else {}
    differs, added = [], []
    cols = META + COUNTED
    for name in args.files:
        old, new = kernels(assembly(args.parent, name, args.hipcc)), kernels(assembly(args.change, name, args.hipcc))
        pretty, pretty_new = demangle(list(old)), demangle(list(new))
        by_pretty = {v: k for k, v in pretty.items()}
        for k, v in pretty_new.items():         # the change's kernel with trailing default arguments stands for the parent's without
            for t in trailing:
                base = re.sub(rf", {re.escape(t)}>\(", ">(", v)
                if k not in old and base != v and base in by_pretty and by_pretty[base] not in new:
                    new[by_pretty[base]] = new.pop(k)
                    break
        lines.append(f"== {name}: {len(old)} kernels in the parent, {len(new)} in the change; totals parent -> change: " +
                     ", ".join(f"{c} {sum(r[c] for r in old.values())} -> {sum(r[c] for r in new.values())}" for c in COUNTED))
        lines.append("   " + " | ".join(("vgpr", "sgpr", "scratch", "lds") + COUNTED) + " | kernel")
        for k in sorted(old, key=lambda k: pretty.get(k, k)):
            if k not in new:
                verdict["missing"].append(k)
                continue
            o, n = old[k], new[k]
            lines.append("   " + " | ".join(str(o[c]) if o[c] == n[c] else f"{o[c]}->{n[c]}" for c in cols) + " | " +
                         pretty.get(k, k).replace("mid::", "").replace("(anonymous namespace)::", "") +
                         (" | same instructions" if o["text"] == n["text"] else " | INSTRUCTIONS DIFFER"))
            if o["text"] != n["text"]: differs.append(k)
            if n["private_segment_fixed_size"] > o["private_segment_fixed_size"]: verdict["scratch"].append(k)
            if n["group_segment_fixed_size"] > o["group_segment_fixed_size"]: verdict["lds"].append(k)
            if waves(n["vgpr_count"]) < waves(o["vgpr_count"]): verdict["waves"].append(k)
            if n["ds_read_b96"] > o["ds_read_b96"] or n["ds_read_b128"] < o["ds_read_b128"]: verdict["b96"].append(k)
        fresh = [k for k in new if k not in old]
        if trailing:                              # new instantiations, with their own figures
            for k in sorted(fresh, key=lambda k: pretty_new.get(k, k)):
                n = new[k]
                lines.append("   " + " | ".join(str(n[c]) for c in cols) + " | NEW " +
                             pretty_new.get(k, k).replace("mid::", "").replace("(anonymous namespace)::", "") + f" | {waves(n['vgpr_count'])} waves per SIMD")
            added += fresh
        else:
            verdict["missing"] += fresh
    lines.append("")
    for key, what in (("missing", "kernels present in one tree only"), ("scratch", "kernels that gained scratch"),
                      ("lds", "kernels that gained static LDS"), ("waves", "kernels in a lower waves-per-SIMD class"),
                      ("b96", "kernels with fewer ds_read_b128 or more ds_read_b96")):
        lines.append(f"{what}: {len(verdict[key])}" + "".join("\n    " + k for k in verdict[key]))
    lines.append(f"kernels whose instructions differ from the parent's: {len(differs)}" + "".join("\n    " + k for k in differs))
    if trailing:
        lines.append(f"new instantiations (listed above as NEW): {len(added)}")
    text = "\n".join(lines) + "\n"
    if args.out:
        open(args.out, "w").write(text)
    sys.stdout.write(text if not args.out else text[text.rindex("\n\n") + 2:])
    return 1 if any(verdict.values()) else 0


if __name__ == "__main__":
    sys.exit(main())
