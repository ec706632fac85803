"""Fold the AUTOINT_TOL / AUTOINT_LOSSES lines of `pytest tests/test_gpu_autoint.py -s` into profiles/autoint_tolerances.txt.

    python -m pytest tests/test_gpu_autoint.py -q -s -m gpu > run.txt;  python tools/autoint_tolerance_report.py run.txt [--out FILE]

Every comparison is counted.  The layer grid's comparisons are folded over the instance count N: per shape and tensor the line of
the worst N is kept, with how many were compared; every other comparison keeps its own line.  (A line may follow pytest's progress
dot on the same output line, so the marker is looked for anywhere in the line.)"""
import argparse
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("log")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "autoint_tolerances.txt"))
    a = ap.parse_args()
    best, order, losses, n, worst = {}, [], [], 0, 0.0
    for line in open(a.log, errors="replace"):
        line = line.rstrip("\n")
        i = line.find("AUTOINT_LOSSES ")
        if i >= 0:
            losses.append(line[i + len("AUTOINT_LOSSES "):])
            continue
        i = line.find("AUTOINT_TOL ")
        m = re.match(r"(.*): ([0-9.e+-]+) \(allowed (.*)\)$", line[i + len("AUTOINT_TOL "):]) if i >= 0 else None
        if not m:
            continue
        n += 1
        what, err, allowed = m.group(1), float(m.group(2)), m.group(3)
        worst = max(worst, err)
        key = re.sub(r"^N=\d+ ", "N=* ", what)
        if key not in best:
            order.append(key)
            best[key] = (err, allowed, what, 1)
        else:
            e, al, w, c = best[key]
            best[key] = (max(e, err), al, w if e >= err else what, c + 1)
    with open(a.out, "w") as f:
        f.write("# AutoInt: the %d comparisons of tests/test_gpu_autoint.py on one MI355X: largest |error| over the tensor's largest entry, "
                "and the bound (largest seen: %.3e).\n" % (n, worst))
        f.write("# Folded by tools/autoint_tolerance_report.py: the layer grid over its instance counts N (the worst N of each shape and "
                "tensor is named, with how many were compared).\n")
        for k in order:
            e, al, w, c = best[k]
            f.write("%s: %.3e (allowed %s)%s\n" % (w, e, al, "" if c == 1 else "  [worst of %d]" % c))
        f.write("# losses of the two optimizer steps per golden: measured (reference)\n")
        for l in losses:
            f.write(l + "\n")
    print("%d comparisons, %d lines, largest error %.3e -> %s" % (n, len(order), worst, a.out))


if __name__ == "__main__":
    main()
