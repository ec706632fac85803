"""Fold the PRM_TOL / PRM_LOSSES lines of `pytest tests/test_gpu_prm.py -s` into profiles/prm_tolerances.txt
(with --prefix SETRANK: the SETRANK_TOL / SETRANK_LOSSES lines of tests/test_gpu_setrank.py into profiles/setrank_tolerances.txt).

    python -m pytest tests/test_gpu_prm.py -q -s -m gpu > run.txt;  python tools/prm_tolerance_report.py run.txt [--prefix PRM] [--out FILE]

Every comparison is counted.  The block grid's comparisons are folded over the number of lists B: per shape and tensor the line of the
B that used the largest share of ITS OWN bound is kept (error and bound of that same comparison), with how many were compared; every
other comparison keeps its own line.  (A line may follow pytest's progress dot on the same output line, so the marker is looked for
anywhere in the line.)"""
import argparse
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("log")
    ap.add_argument("--prefix", default="PRM", help="the marker of the lines: PRM or SETRANK")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    name, tol, loss = a.prefix.lower(), a.prefix + "_TOL ", a.prefix + "_LOSSES "
    a.out = a.out or os.path.join(ROOT, "profiles", name + "_tolerances.txt")
    best, order, losses, n, worst, share = {}, [], [], 0, 0.0, 0.0
    for line in open(a.log, errors="replace"):
        line = line.rstrip("\n")
        i = line.find(loss)
        if i >= 0:
            losses.append(line[i + len(loss):])
            continue
        i = line.find(tol)
        m = re.match(r"(.*): ([0-9.e+-]+) \(allowed (.*)\)$", line[i + len(tol):]) if i >= 0 else None
        if not m:
            continue
        n += 1
        what, err, allowed = m.group(1), float(m.group(2)), m.group(3)
        worst = max(worst, err)
        used = err / float(allowed.split(":")[0])
        share = max(share, used)
        key = re.sub(r"^B=\d+ ", "B=* ", what)
        if key not in best:
            order.append(key)
            best[key] = (used, err, allowed, what, 1)
        else:
            u, e, al, w, c = best[key]
            best[key] = ((used, err, allowed, what) if used > u else (u, e, al, w)) + (c + 1,)
    with open(a.out, "w") as f:
        f.write("# %s: the %d comparisons of tests/test_gpu_%s.py on one MI355X: largest |error| over the tensor's largest entry, and "
                "the bound (largest error seen: %.3e; largest share of a bound used: %.2f).\n" % (a.prefix, n, name, worst, share))
        f.write("# Folded by tools/prm_tolerance_report.py: the block grid over its list counts B (the B of each shape and tensor that "
                "used most of its own bound is named, with how many were compared).\n")
        for k in order:
            _, e, al, w, c = best[k]
            f.write("%s: %.3e (allowed %s)%s\n" % (w, e, al, "" if c == 1 else "  [worst of %d]" % c))
        f.write("# losses of the two optimizer steps per golden: measured (reference)\n")
        for l in losses:
            f.write(l + "\n")
    print("%d comparisons, %d lines, largest error %.3e -> %s" % (n, len(order), worst, a.out))


if __name__ == "__main__":
    main()
