"""A/B of two library builds over the project's timing tools, judged against the parent-against-parent spread:

    python tools/ab_parent_change.py --parent parent/libmi_denoise.so --change image_denoising_filter_amd/libmi_denoise.so \
           [--rounds 5] --out profiles/rNN_ab.txt tool [tool ...]          (tools: the keys of TOOLS below)

The parent runs as two series, Pa and Pb (the same file), the change as C; every round runs Pa, C, Pb, each in a fresh process
(MID_LIB_PATH).  Per time figure a tool prints (ms, lower is better) the table gives the medians over the rounds, the spread
|median Pa - median Pb|, and marks the figure SLOWER when median C > median of all parent runs + spread.  Stops at the first
run that does not exit 0.  `bench_full` compares the "ms" entries of one `bench.py --full` line per run.
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

TOOLS = {
    "ab_bil": ["tools/ab_bil.py", "x"],
    "ab_bil_layout": ["tools/ab_bil_layout.py"],
    "bil_rt_time": ["tools/bil_rt_time.py"],
    "layers_time": ["tools/layers_time.py"],
    "nlm_layers_rate": ["tools/nlm_layers_rate.py", "--rounds", "3", "--reps", "5"],
    "nlm_layers_rate_untuned": ["tools/nlm_layers_rate.py", "--rounds", "3", "--reps", "5", "--untuned"],   # + the per-pixel kernels
    "bilateral_temporal_rate": ["tools/bilateral_temporal_rate.py", "--rounds", "3", "--reps", "5", "--frames", "32"],
    "nlm_layers_temporal_rate": ["tools/nlm_layers_temporal_rate.py", "--rounds", "3", "--reps", "3", "--frames", "16"],
    "bench_full": ["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "3", "--full", "--no-cpu-baseline"],
}
# table rows of the rate tools (every token a number or 'plain'): name of the row from its first tokens, and the time columns
ROWS = {"nlm_layers_rate": (("L",), {1: "fused", 4: "chain"}),
        "nlm_layers_rate_untuned": (("L",), {1: "fused", 4: "chain"}),
        "bilateral_temporal_rate": (("k", "L"), {3: "fused", 6: "chain"}),
        "nlm_layers_temporal_rate": (("k", "L"), {3: "fused", 6: "chain"})}
NUM = re.compile(r"^-?\d+(\.\d+)?$")


def walk_ms(node, path, out):
    if isinstance(node, dict):
        for k, v in node.items():
            if isinstance(v, (int, float)) and not isinstance(v, bool) and (k == "ms" or k.startswith("ms_per") or k.endswith("_ms")):
                out.append((".".join(path + [k]), float(v)))
            else:
                walk_ms(v, path + [k], out)


def figures(tool, text):
    """[(label, ms)] of one run's output."""
    out = []
    if tool == "bench_full":
        line = [l for l in text.splitlines() if l.startswith("{")][-1]
        walk_ms(json.loads(line), [], out)
        return out
    lines = text.splitlines()
    if tool == "ab_bil":
        lines = [l.replace("variant x", "") for l in lines if l.startswith("variant")][-1:]      # the warm repetition
    section = ""
    for line in lines:
        toks = line.split()
        if toks and tool in ROWS and all(NUM.match(t) or t == "plain" for t in toks):
            keys, cols = ROWS[tool]
            name = " ".join(f"{k}={t}" for k, t in zip(keys, toks))
            out += [(f"{section}: {name} {what}", float(toks[i])) for i, what in cols.items()]
            continue
        if line.strip() and not line.startswith(" "):
            section = re.split(r"[:(]", line.strip())[0].strip()[:32]
        for m in re.finditer(r"(-?\d+\.\d+) ms", line):
            before = re.split(r"[|;]|\)\s+", line[:m.start()])[-1].strip(" :,")
            before = re.sub(r"-?\d+\.\d+ ms.*?, ", "", before)
            label = before[-44:] if before else section
            out.append((label if label.startswith(section) or tool in ("ab_bil", "bil_rt_time", "layers_time", "ab_bil_layout") else f"{section}: {label}",
                        float(m.group(1))))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--change", required=True)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", required=True)
    ap.add_argument("tools", nargs="+", choices=list(TOOLS))
    args = ap.parse_args()
    libs = {"Pa": args.parent, "Pb": args.parent, "C": args.change}
    log = open(args.out, "w")

    def say(s=""):
        print(s, flush=True)
        log.write(s + "\n")
        log.flush()

    say(f"parent (two series of the same library, Pa and Pb) against change (C): {args.rounds} rounds of Pa, C, Pb per tool, a fresh process per run.")
    say("Times in ms, medians over the rounds.  spread = |median Pa - median Pb|; SLOWER = median C > median of all parent runs + spread.")
    failed = []
    for tool in args.tools:
        res = {k: [] for k in libs}
        t0 = time.time()
        for rnd in range(1 if tool == "bench_full" else args.rounds):
            for key in ("Pa", "C", "Pb"):
                env = dict(os.environ, MID_LIB_PATH=os.path.abspath(libs[key]))
                r = subprocess.run([sys.executable, *TOOLS[tool]], env=env, capture_output=True, text=True, timeout=420)
                if r.returncode != 0:
                    say(f"{tool} {key} round {rnd}: exit {r.returncode}\n{r.stdout[-1500:]}\n{r.stderr[-1500:]}")
                    return 1
                res[key].append(figures(tool, r.stdout))
        say(f"\n== {tool} ({' '.join(TOOLS[tool])}; {time.time() - t0:.0f} s)")
        say(f"   {'Pa':>9} {'Pb':>9} {'parent':>9} {'C':>9} {'spread':>8} {'C/parent':>8}  figure")
        n = len(res["Pa"][0])
        if not all(len(run) == n for runs in res.values() for run in runs):
            say("the runs printed different numbers of figures")
            return 1
        for i in range(n):
            med = {k: statistics.median(run[i][1] for run in res[k]) for k in libs}
            parent = statistics.median([run[i][1] for run in res["Pa"]] + [run[i][1] for run in res["Pb"]])
            spread = abs(med["Pa"] - med["Pb"])
            ok = med["C"] <= parent + spread
            label = res["Pa"][0][i][0]
            if not ok:
                failed.append((tool, label, parent, med["C"], spread))
            say(f"   {med['Pa']:9.4f} {med['Pb']:9.4f} {parent:9.4f} {med['C']:9.4f} {spread:8.4f} {med['C'] / parent if parent else 0:8.4f}  {'' if ok else 'SLOWER '}{label}")
    say(f"\nfigures where the change's median is slower than the parent's by more than the spread: {len(failed)}")
    for f in failed:
        say(f"   {f[0]}: {f[1]}: parent {f[2]:.4f} change {f[3]:.4f} spread {f[4]:.4f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
