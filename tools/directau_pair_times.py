"""Per-shape time of DirectAU's pairwise kernel from a rocprofv3 kernel trace of tools/bench_directau.py; prints ONE JSON line.

    rocprofv3 --kernel-trace --stats -d DIR -o kt --output-format csv -- python tools/bench_directau.py --shapes S ...
    python tools/directau_pair_times.py DIR/kt_kernel_trace.csv --shapes S [--bench bench.json]

Each dispatch of dau_pair_kernel<DP> is matched to its shape by the kernel's DP (d rounded up to 32) and its grid (256 threads
per 128 rows of the batch).  Per shape: dispatch count, median / min duration, algorithmic TFLOP/s (3 d B (B - 1) per set, both
sets) and their fraction of the 157.3 TF fp32 MFMA peak at the median; with --bench (the JSON line bench_directau.py printed), the
torch formulation's time over the median as well.
"""
import argparse
import csv
import json
import re
import statistics

PEAK_FLOPS = 157.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--shapes", default="256x64,4096x64,65536x64,4096x128")
    ap.add_argument("--bench", default="")
    a = ap.parse_args()
    durations = {}
    with open(a.trace) as f:
        for row in csv.DictReader(f):
            m = re.search(r"dau_pair_kernel<(\d+)>", row["Kernel_Name"])
            if m:
                key = (int(m.group(1)), int(row["Grid_Size_X"]))
                durations.setdefault(key, []).append(int(row["End_Timestamp"]) - int(row["Start_Timestamp"]))
    bench = json.load(open(a.bench))["shapes"] if a.bench else {}
    out = {"source": "rocprofv3 --kernel-trace, dau_pair_kernel dispatches", "peak_fp32_mfma_tflops": PEAK_FLOPS / 1e12,
           "shapes": {}}
    for s in a.shapes.split(","):
        B, d = (int(x) for x in s.split("x"))
        ns = durations.get(((d + 31) // 32 * 32, (B + 127) // 128 * 256), [])
        if not ns:
            out["shapes"][s] = None
            continue
        med = statistics.median(ns) * 1e-9
        flops = 2 * 3.0 * d * B * (B - 1)
        r = {"dispatches": len(ns), "pair_kernel_ms_median": round(med * 1e3, 4), "pair_kernel_ms_min": round(min(ns) * 1e-6, 4),
             "algorithmic_tflops": round(flops / med / 1e12, 2), "fraction_of_mfma_peak": round(flops / med / PEAK_FLOPS, 3)}
        t = bench.get(s, {}).get("torch_ms")
        if t:
            r["torch_ms_over_pair_kernel"] = round(t / (med * 1e3), 1)
        out["shapes"][s] = r
    print(json.dumps(out))


if __name__ == "__main__":
    main()
