"""Weather-year resources on the HL1 sequential chronology (relmc_hl1_var_seq) on RTS-24, on hl1_seq_rate.py's shape (a): 2e5 one-year
chains, stationary start.  One process: after a warm-up of every variant, relmc_hl1_seq, relmc_hl1_seq_storage without storage and
relmc_hl1_var_seq with 0, 2 and 8 resources without storage and with 2 resources plus one 100 MW / 400 MWh battery at 0.92 / 0.92 are
timed in turn (REPS rounds); kernel time is relmc_last_kernel_ms.  The library is hl1_variable.synthetic_weather's (5 weather years, RANDOM
pick, no load curves of its own; the 8 resources are its solar and wind four times over at a quarter of the nameplate).  Prints the
best, the median and the spread of every variant and the ratio of the best times to relmc_hl1_seq_storage's of the same run: that
kernel's code object does not change with this unit, so it is the yardstick.
  python scripts/hl1_variable_rate.py [--chains N] [--reps R]"""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATTERY = [(100.0, 100.0, 400.0, 0.92, 0.92, 400.0)]
YARDSTICK = "storage call, no storage"


def device_rates(chains, reps):
    from powersystemsreliabilityassessment_amd import _abi, _lib, api, case24, hl1, hl1_variable
    gens, load = hl1.rts24_generators(), hl1.rts24_load()
    eng = api.Engine(case24.rts24(), device=0)
    hl1._seq_model_load(eng, gens, load)
    start = _abi.HL1_START_STATIONARY
    two = hl1_variable.synthetic_weather(5, hours=load.hourly_load.size, solar_mw=300.0, wind_mw=300.0)
    libs = {0: hl1_variable.WeatherYears(np.zeros((5, 0, two.hours))), 2: two,
            8: hl1_variable.WeatherYears(np.ascontiguousarray(np.tile(two.output_mw * 0.25, (1, 4, 1))))}

    def seq(seed):
        acc = _abi.Hl1SeqAcc()
        eng._check(eng.L.relmc_hl1_seq(eng._h, seed, 0, chains, 1, start, C.byref(acc), None), "relmc_hl1_seq")
        return eng.last_kernel_ms(), acc

    def storage(seed):
        acc = _abi.Hl1StorageAcc()
        eng._check(eng.L.relmc_hl1_seq_storage(eng._h, seed, 0, chains, 1, start, 1.0, 0.0, 0, None, C.byref(acc), None, None), "relmc_hl1_seq_storage")
        return eng.last_kernel_ms(), acc

    def variable(seed, nres, st):
        hl1_variable._weather_load(eng, libs[nres])
        opts = _abi.Hl1VarOpts()
        for r in range(nres):
            opts.resource_scale[r] = 1.0
        opts.scale, opts.shift, opts.pick = 1.0, 0.0, _abi.HL1_VAR_PICK_RANDOM
        arr = (_abi.Hl1Storage * max(len(st), 1))(*[_abi.Hl1Storage(*s) for s in st])
        acc = _abi.Hl1StorageAcc()
        eng._check(eng.L.relmc_hl1_var_seq(eng._h, seed, 0, chains, 1, start, C.byref(opts), len(st), arr if st else None, C.byref(acc), None, None, None),
                   "relmc_hl1_var_seq")
        return eng.last_kernel_ms(), acc

    variants = (("relmc_hl1_seq", seq), (YARDSTICK, storage),
                ("var, 0 resources", lambda s: variable(s, 0, [])), ("var, 2 resources", lambda s: variable(s, 2, [])),
                ("var, 8 resources", lambda s: variable(s, 8, [])), ("var, 2 resources + battery", lambda s: variable(s, 2, BATTERY)))
    for _, fn in variants:                                 # warm-up: code objects, buffers
        fn(1)
    ms = {name: [] for name, _ in variants}
    accs = {}
    for r in range(reps):
        for name, fn in variants:
            t, accs[name] = fn(1 + r)
            ms[name].append(t)
    base = min(ms[YARDSTICK])
    print(f"{chains} chains x 1 year, stationary, RTS-24; code object {_lib.code_object_sha256()[:12]}; kernel time = relmc_last_kernel_ms", flush=True)
    for name, v in ms.items():
        print(f"  {name:27s} best {min(v):8.3f} ms  median {statistics.median(v):8.3f}  max {max(v):8.3f}  (n = {len(v)})  "
              f"best / best of the yardstick {min(v) / base:.3f}", flush=True)
    print(f"  spread of the yardstick's repeats: {min(ms[YARDSTICK]) / base:.3f} .. {max(ms[YARDSTICK]) / base:.3f}", flush=True)
    for name, a in accs.items():
        line = f"  {name:27s} LOLE {a.sum_lole / a.years:.4f} h/yr  EUE {a.sum_eue / a.years:.2f} MWh/yr  LOLF {a.sum_lolf / a.years:.4f}"
        if hasattr(a, "sum_served"):
            line += f"  served {a.sum_served / a.years:.4f} h/yr  discharged {a.sum_discharged / a.years:.2f}  charged {a.sum_charged / a.years:.2f} MWh/yr"
        print(line, flush=True)
    eng.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=200000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    device_rates(a.chains, a.reps)
