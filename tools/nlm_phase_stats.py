#!/usr/bin/env python3
"""Figures of one distance phase of an NLM strip kernel, read from the compiler's assembly listing.

    hipcc <the Makefile's flags for nlm.hip> --cuda-device-only -S csrc/nlm.hip -o nlm.s
    tools/nlm_phase_stats.py nlm.s [mangled-name substring, default: the bench kernel]

A distance phase is what lies between the drop of the issue priority (s_setprio 0) and the next raise (s_setprio 1) in
straight-line code.  Printed: the kernel's VGPRs and scratch, the static VALU count of the whole kernel, and for the phases
the VALU count, the number of v_fma_f32 / v_fmac_f32 whose addend is the result of an earlier v_fma_f32 / v_fmac_f32 of the phase (the running-sum
chains) and the smallest / median distance, in instructions, between such a pair."""
import re
import statistics
import sys

BENCH = "nlm_strip_kernelILin10ELi11ELin3ELi4ELi8ELi4ELi0ELb1ELb0ELb0ELi0EE"


def kernel_text(lines, key):
    start = next(i for i, l in enumerate(lines) if l.startswith("_Z") and key in l and l.rstrip().split(":")[0].endswith("E"))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith("\t.end_amdhsa_kernel") or ".end_amdhsa_kernel" in lines[i])
    return lines[start:end]


def main():
    path = sys.argv[1]
    key = sys.argv[2] if len(sys.argv) > 2 else BENCH
    text = kernel_text(open(path).read().split("\n"), key)
    meta = {}
    for l in text:
        m = re.match(r"\s*[;.]\s*(NumVgprs|ScratchSize|Occupancy|\.?amdhsa_next_free_vgpr)\W+(\d+)", l)
        if m:
            meta[m.group(1)] = int(m.group(2))
    ins = [l.split(";")[0].split() for l in text if l.startswith("\t") and not l.startswith("\t.") and not l.startswith("\t;")]
    ins = [t for t in ins if t]
    valu_all = sum(1 for t in ins if t[0].startswith("v_"))
    print(f"kernel {key}: {meta}  static VALU {valu_all}")
    phases, cur = [], None
    for t in ins:
        if t[0] == "s_setprio":
            if t[1] == "0":
                cur = []
            elif cur is not None:
                phases.append(cur)
                cur = None
        elif cur is not None:
            if t[0].startswith("s_cbranch") or t[0] == "s_branch":
                cur = None  # not straight-line: the end of a run
            else:
                cur.append(t)
    rows = []
    for ph in phases:
        valu = [t for t in ph if t[0].startswith("v_")]
        last_fma = {}  # destination register -> index among the phase's VALU instructions
        dist = []
        for i, t in enumerate(valu):
            ops = [o.rstrip(",") for o in t[1:]]
            fma = t[0] == "v_fma_f32" or t[0].startswith("v_fmac_f32")
            addend = ops[3] if t[0] == "v_fma_f32" and len(ops) >= 4 else ops[0] if fma else None   # (v_fmac: the destination)
            if addend in last_fma:
                dist.append(i - last_fma[addend])
            if ops:
                last_fma.pop(ops[0], None)
                if fma:
                    last_fma[ops[0]] = i
        rows.append((len(valu), len(dist), min(dist) if dist else 0, statistics.median(dist) if dist else 0,
                     sum(1 for t in ph if t[0].startswith("ds_read"))))
    if not rows:
        print("no distance phase found")
        return
    full = [r for r in rows if r[0] >= statistics.median([x[0] for x in rows]) - 2]
    print(f"{len(rows)} distance phases in straight-line code; per phase (median over the {len(full)} full ones): "
          f"VALU {statistics.median([r[0] for r in full])}, chained FMAs {statistics.median([r[1] for r in full])}, "
          f"dependent-FMA distance min {min(r[2] for r in full)} (median of phase minima {statistics.median([r[2] for r in full])}, "
          f"median distance {statistics.median([r[3] for r in full])}), ds_read {statistics.median([r[4] for r in full])}")


if __name__ == "__main__":
    main()
