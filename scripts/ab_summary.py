"""Summary of a same-session A/B record (profiles/<name>/ab_runs.txt -> ab_summary.txt):
    python scripts/ab_summary.py profiles/<name>/ab_runs.txt > profiles/<name>/ab_summary.txt
Lines of the record: `<label> <build> rep <k> kernel_ms_avg <ms> value <v> ...`; the first build of a label is its parent.  Per label and
build: the runs, their median and spread (max - min), the gap to the parent's median and gap / (the larger spread of the pair), and the
verdict of the project's rule: FASTER only if the median kernel time is below the parent's by at least 5 x the larger spread and `value`
moves the same way; SLOWER by the mirror image; else "not told apart by the rule"."""
import collections, statistics, sys

runs = collections.OrderedDict()
for ln in open(sys.argv[1]):
    w = ln.split()
    if len(w) < 8 or w[2] != "rep":
        continue
    runs.setdefault(w[0], collections.OrderedDict()).setdefault(w[1], []).append((float(w[w.index("kernel_ms_avg") + 1]), float(w[w.index("value") + 1])))
for label, builds in runs.items():
    parent = next(iter(builds))
    pk = [k for k, _ in builds[parent]]
    pmed, pspread, pval = statistics.median(pk), max(pk) - min(pk), statistics.median(v for _, v in builds[parent])
    for b, r in builds.items():
        k = [x for x, _ in r]
        med, spread, val = statistics.median(k), max(k) - min(k), statistics.median(v for _, v in r)
        big = max(spread, pspread)
        verdict = "" if b == parent else ("  FASTER" if pmed - med >= 5 * big and val > pval else ("  SLOWER" if med - pmed >= 5 * big and val < pval else "  not told apart by the rule"))
        print("%-26s %-10s kernel_ms_avg runs %s median %.4f (%+.3f ms, %+.2f %%)  spread %.4f (larger of the pair %.4f, gap/spread %.1f)  value median %.5g (%+.2f %%)%s"
              % (label, b, " ".join("%.4f" % x for x in k), med, med - pmed, 100 * (med - pmed) / pmed, spread, big, abs(med - pmed) / big if big else 0.0, val, 100 * (val - pval) / pval, verdict))
