"""Host-only count behind kNormSplitMask (csrc/relmc_kernels.hip): on what share of a wavefront's trips through the interior-point loop does
NO row pass the first stage of the convergence test (complementarity and cost change), so that the trip needs none of the four second-stage
termination norms?
    python scripts/norm_trip_model.py [n_states] [seed]          (default 400 1)
The numpy oracle's mips_lp (oracle/pyoracle.py) is run on the first n sampled RTS-24 states of the seed under REFERENCE_EMULATE, from a copy of
its source text in which the four conditions are recorded after every iteration (nothing under oracle/ is changed).  A wavefront = four
consecutive samples, no window sorting; it runs trips 0 .. max(iterations of its rows), a row takes part in trips 0 .. its own iteration
count, and trip 0 (the start point) never needs the norms.  Also printed: the same share with the cost test alone as the gate, and the first
iteration at which each gate passes.  The kernel's own count comes from a -DRELMC_PHASE_TIMING build (scripts/phase_timing.py)."""
import collections, inspect, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from oracle import coracle, pyoracle
from powersystemsreliabilityassessment_amd import case24

n = int(sys.argv[1]) if len(sys.argv) > 1 else 400
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1

LINE = "feas, grad, comp, cost = conds(x, z, lam, mu, g, h, Lx, f, f0)"
src = inspect.getsource(pyoracle.mips_lp)
assert src.count(LINE) == 2, "mips_lp no longer evaluates its conditions where this script expects them"
ns = dict(vars(pyoracle)); ns["_TRACE"] = []
exec(src.replace(LINE, LINE + "; _TRACE.append((feas, grad, comp, cost))"), ns)
mips_traced, trace = ns["mips_lp"], ns["_TRACE"]

case = case24.rts24()
states = pyoracle.mc_sampling(coracle.Oracle(case).thresholds(), seed, 0, n)
tol = pyoracle.MIPS_DEFAULTS
rows = []          # per state: (iterations, [first stage passes after iteration t], [cost test alone passes])
for st in states:
    lp = pyoracle.build_lp(case, st, pyoracle.REFERENCE_EMULATE)
    if lp["pre"]["singular"]:
        rows.append((0, [False], [False])); continue
    del trace[:]
    _, _, eflag, it = mips_traced(lp["c"], lp["A"], lp["l"], lp["u"], lp["xmin"], lp["xmax"], lp["x0"])
    assert len(trace) == it + 1
    s1 = [t > 0 and c[2] < tol["comptol"] and c[3] < tol["costtol"] for t, c in enumerate(trace)]
    sc = [t > 0 and c[3] < tol["costtol"] for t, c in enumerate(trace)]
    rows.append((it, s1, sc))

print("iteration counts:", sorted(collections.Counter(r[0] for r in rows).items()))
first = lambda flags: next((t for t, f in enumerate(flags) if f), None)
print("first iteration with the first stage passed, minus the converging iteration:",
      sorted(collections.Counter(first(r[1]) - r[0] for r in rows if r[0] and first(r[1]) is not None).items()))
print("first iteration with the cost test passed:", sorted(collections.Counter(first(r[2]) for r in rows if r[0]).items()))
for name, k in (("first stage (complementarity and cost)", 1), ("cost test alone", 2)):
    trips = free = 0
    for g in range(0, len(rows) - len(rows) % 4, 4):
        grp = rows[g:g + 4]
        for t in range(max(r[0] for r in grp) + 1):
            need = any(t <= r[0] and t < len(r[k]) and r[k][t] for r in grp)
            trips += 1; free += not need
    print(f"gate = {name}: {free} of {trips} wavefront trips need no second-stage norm ({free / trips:.4f})")
