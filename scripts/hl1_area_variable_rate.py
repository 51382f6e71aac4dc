"""Weather-year resources and storages in the areas of the multi-area chronology (relmc_hl1_area_var) on hl1_area_rate.py's shapes
(a) RTS-96 and (c) the demo system, both INTERCONNECTED, 2e5 one-year chains, stationary start, flow "reference".  One process per shape:
after a warm-up of every variant, relmc_hl1_area and four forms of relmc_hl1_area_var -- nothing added, two resources, eight resources,
two resources plus one 100 MW / 400 MWh battery at 0.92 / 0.92 per area -- are timed in turn (REPS rounds); kernel time is
relmc_last_kernel_ms.  The library is hl1_variable.synthetic_weather's (5 weather years, RANDOM pick, no load curves of its own; the
resources go round the areas; the 8 resources are its solar and wind four times over at a quarter of the nameplate).  Prints the best,
the median and the spread of every variant and the ratio of the medians to relmc_hl1_area's of the same run: that kernel's code object
does not change with this unit, so it is the yardstick.
  python scripts/hl1_area_variable_rate.py [--case a|c] [--chains N] [--reps R]     without --case: both, each in a child process"""
import argparse
import ctypes as C
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATTERY = (100.0, 100.0, 400.0, 0.92, 0.92, 400.0)
YARDSTICK = "relmc_hl1_area"


def device_rates(case, chains, reps):
    from powersystemsreliabilityassessment_amd import _abi, _lib, api, case24, hl1_area_variable as AV, hl1_areas, hl1_variable
    sysm = hl1_areas.rts96_system() if case == "a" else hl1_areas.demo_system()
    n = len(sysm.areas)
    eng = api.Engine(case24.rts24(), device=0)
    units, cap, mttf, mttr, load, tf, tt, tc = hl1_areas._flatten(sysm)
    hl1_areas._model_load(eng, units, cap, mttf, mttr, load, tf, tt, tc, None, None)
    start, policy, flow = _abi.HL1_START_STATIONARY, _abi.HL1_AREA_INTERCONNECTED, _abi.HL1_AREA_FLOW_REFERENCE
    two = hl1_variable.synthetic_weather(5, hours=load.shape[1], solar_mw=300.0, wind_mw=300.0)
    area_of = lambda k: tuple(r % n + 1 for r in range(k))
    libs = {0: AV.AreaWeatherYears(np.zeros((5, 0, two.hours)), ()), 2: AV.AreaWeatherYears(two.output_mw, area_of(2)),
            8: AV.AreaWeatherYears(np.ascontiguousarray(np.tile(two.output_mw * 0.25, (1, 4, 1))), area_of(8))}

    def area(seed):
        acc = (_abi.Hl1SeqAcc * (n + 1))()
        eng._check(eng.L.relmc_hl1_area(eng._h, seed, 0, chains, 1, start, policy, flow, acc, None), "relmc_hl1_area")
        return eng.last_kernel_ms(), acc

    def variable(seed, nres, batteries):
        AV._library_load(eng, libs[nres], n)
        opts = _abi.Hl1AreaVarOpts()
        for a in range(_abi.AREA_MAX):
            opts.load_scale[a] = 1.0
        for r in range(nres):
            opts.resource_scale[r] = 1.0
        opts.policy, opts.flow, opts.pick = policy, flow, _abi.HL1_VAR_PICK_RANDOM
        ns = n if batteries else 0
        arr = (_abi.Hl1AreaStorage * max(ns, 1))()
        for a in range(ns):
            arr[a].s, arr[a].area = _abi.Hl1Storage(*BATTERY), a
        acc = (_abi.Hl1StorageAcc * (n + 1))()
        eng._check(eng.L.relmc_hl1_area_var(eng._h, seed, 0, chains, 1, start, C.byref(opts), ns, arr if ns else None, acc, None, None, None),
                   "relmc_hl1_area_var")
        return eng.last_kernel_ms(), acc

    variants = ((YARDSTICK, area), ("area_var, nothing added", lambda s: variable(s, 0, False)), ("area_var, 2 resources", lambda s: variable(s, 2, False)),
                ("area_var, 8 resources", lambda s: variable(s, 8, False)), ("area_var, 2 resources + batteries", lambda s: variable(s, 2, True)))
    for _, fn in variants:                                 # warm-up: code objects, buffers
        fn(1)
    ms = {name: [] for name, _ in variants}
    accs = {}
    for r in range(reps):
        for name, fn in variants:
            t, accs[name] = fn(1 + r)
            ms[name].append(t)
    base = statistics.median(ms[YARDSTICK])
    print(f"({case}) {'RTS-96' if case == 'a' else 'demo'}, {chains} chains x 1 year, stationary, INTERCONNECTED; code object "
          f"{_lib.code_object_sha256()[:12]}; kernel time = relmc_last_kernel_ms", flush=True)
    for name, v in ms.items():
        print(f"  {name:34s} best {min(v):8.3f} ms  median {statistics.median(v):8.3f}  max {max(v):8.3f}  (n = {len(v)})  "
              f"median / median of the yardstick {statistics.median(v) / base:.3f}", flush=True)
    print(f"  spread of the yardstick's repeats: {min(ms[YARDSTICK]) / base:.3f} .. {max(ms[YARDSTICK]) / base:.3f}", flush=True)
    for name, a in accs.items():
        s = a[n]
        line = f"  {name:34s} system LOLE {s.sum_lole / s.years:.4f} h/yr  EUE {s.sum_eue / s.years:.2f} MWh/yr  LOLF {s.sum_lolf / s.years:.4f}"
        if hasattr(s, "sum_served"):
            line += f"  served {s.sum_served / s.years:.4f} h/yr  discharged {s.sum_discharged / s.years:.2f}  charged {s.sum_charged / s.years:.2f} MWh/yr"
        print(line, flush=True)
    eng.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=("a", "c"))
    ap.add_argument("--chains", type=int, default=200000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if a.case:
        device_rates(a.case, a.chains, a.reps)
        sys.exit(0)
    for case in ("a", "c"):
        rc = subprocess.call(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--case", case, "--chains", str(a.chains),
                              "--reps", str(a.reps)])
        if rc != 0:
            print(f"case ({case}) ended with status {rc}; no further GPU case is started", flush=True)
            sys.exit(1)
