"""Weather-dependent forced outage rates on the HL1 sequential chronology (relmc_hl1_stress_seq) on RTS-24, on hl1_variable_rate.py's shape:
2e5 one-year chains, stationary start, hl1_variable.synthetic_weather's library (5 weather years with load curves of their own, solar and
wind, RANDOM pick).  One process: after a warm-up of every variant, relmc_hl1_var_seq and relmc_hl1_stress_seq with every unit in class
-1, with every unit stressed at multiplier 1 and with hl1_stress.synthetic_stress are timed in turn (REPS rounds), without storage and
with one 100 MW / 400 MWh battery at 0.92 / 0.92; kernel time is relmc_last_kernel_ms.  Prints the best, the median and the spread of
every variant and the ratio of the best times to relmc_hl1_var_seq's with the same storages in the same run: that kernel's code object
does not change with this unit, so it is the yardstick.
  python scripts/hl1_stress_rate.py [--chains N] [--reps R]"""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATTERY = [(100.0, 100.0, 400.0, 0.92, 0.92, 400.0)]


def device_rates(chains, reps):
    from powersystemsreliabilityassessment_amd import _abi, _lib, api, case24, hl1, hl1_stress, hl1_variable
    gens, load = hl1.rts24_generators(), hl1.rts24_load()
    eng = api.Engine(case24.rts24(), device=0)
    hl1._seq_model_load(eng, gens, load)
    start = _abi.HL1_START_STATIONARY
    W = hl1_variable.synthetic_weather(5, hours=load.hourly_load.size, solar_mw=300.0, wind_mw=300.0, load=load)
    hl1_variable._weather_load(eng, W)
    syn = hl1_stress.synthetic_stress(W, load, gens)
    K = len(gens)
    libs = {"class -1": hl1_stress.OutageStress(syn.fail_mult, np.full(K, -1)),
            "multiplier 1": hl1_stress.OutageStress(np.ones_like(syn.fail_mult), syn.unit_class),
            "synthetic": syn}

    def call(fn, name, seed, st):
        opts = _abi.Hl1VarOpts()
        opts.resource_scale[0] = opts.resource_scale[1] = 1.0
        opts.scale, opts.shift, opts.pick = 1.0, 0.0, _abi.HL1_VAR_PICK_RANDOM
        arr = (_abi.Hl1Storage * max(len(st), 1))(*[_abi.Hl1Storage(*s) for s in st])
        acc = _abi.Hl1StorageAcc()
        eng._check(fn(eng._h, seed, 0, chains, 1, start, C.byref(opts), len(st), arr if st else None, C.byref(acc), None, None, None), name)
        return eng.last_kernel_ms(), acc

    def stress(lib, seed, st):
        hl1_stress._stress_load(eng, libs[lib])
        return call(eng.L.relmc_hl1_stress_seq, "relmc_hl1_stress_seq", seed, st)

    variants = []
    for tag, st in (("", []), (" + battery", BATTERY)):
        variants.append(("relmc_hl1_var_seq" + tag, tag, lambda s, st=st: call(eng.L.relmc_hl1_var_seq, "relmc_hl1_var_seq", s, st)))
        for lib in libs:
            variants.append((f"stress, {lib}{tag}", tag, lambda s, lib=lib, st=st: stress(lib, s, st)))
    for _, _, fn in variants:                              # warm-up: code objects, buffers
        fn(1)
    ms = {name: [] for name, _, _ in variants}
    accs = {}
    for r in range(reps):
        for name, _, fn in variants:
            t, accs[name] = fn(1 + r)
            ms[name].append(t)
    print(f"{chains} chains x 1 year, stationary, RTS-24, 2 resources; code object {_lib.code_object_sha256()[:12]}; kernel time = relmc_last_kernel_ms",
          flush=True)
    for name, tag, _ in variants:
        v, base = ms[name], min(ms["relmc_hl1_var_seq" + tag])
        print(f"  {name:34s} best {min(v):8.3f} ms  median {statistics.median(v):8.3f}  max {max(v):8.3f}  (n = {len(v)})  "
              f"best / best of relmc_hl1_var_seq{tag} {min(v) / base:.3f}", flush=True)
    for tag in ("", " + battery"):
        v = ms["relmc_hl1_var_seq" + tag]
        print(f"  spread of relmc_hl1_var_seq{tag}'s repeats: 1.000 .. {max(v) / min(v):.3f}", flush=True)
    for name, a in accs.items():
        print(f"  {name:34s} LOLE {a.sum_lole / a.years:.4f} h/yr  EUE {a.sum_eue / a.years:.2f} MWh/yr  LOLF {a.sum_lolf / a.years:.4f}  "
              f"served {a.sum_served / a.years:.4f} h/yr", flush=True)
    eng.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=200000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    device_rates(a.chains, a.reps)
