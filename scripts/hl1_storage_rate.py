"""Energy storage on the HL1 sequential chronology (relmc_hl1_seq_storage) on RTS-24 against relmc_hl1_seq, on hl1_seq_rate.py's shape
(a): 2e5 one-year chains, stationary start.  One process, one call: after a warm-up of every variant, relmc_hl1_seq and
relmc_hl1_seq_storage are timed alternately (REPS rounds), the storage call with no storage, with one 100 MW / 400 MWh battery at
0.92 / 0.92, and with eight storages; kernel time is relmc_last_kernel_ms.  Prints the median, the spread and the ratio to relmc_hl1_seq
of the same run, then the share of 64-step groups that take the kernel's serial stage, counted on the host model for the same fleet.
  python scripts/hl1_storage_rate.py [--chains N] [--reps R] [--host-chains M]      (--host-chains 0: no host count)"""
import argparse
import ctypes as C
import importlib.util
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATTERY = [(100.0, 100.0, 400.0, 0.92, 0.92, 400.0)]
# eight unlike storages, 300 MW / 1220 MWh in all
EIGHT = [(100.0, 100.0, 400.0, 0.92, 0.92, 400.0), (50.0, 50.0, 100.0, 0.95, 0.95, 100.0), (40.0, 40.0, 320.0, 0.85, 0.9, 160.0),
         (30.0, 30.0, 60.0, 0.9, 0.9, 0.0), (25.0, 25.0, 100.0, 1.0, 1.0, 100.0), (20.0, 20.0, 80.0, 0.8, 0.8, 80.0),
         (20.0, 20.0, 40.0, 0.92, 0.92, 40.0), (15.0, 15.0, 120.0, 0.75, 0.95, 60.0)]
VARIANTS = (("no storage", []), ("one battery", BATTERY), ("eight storages", EIGHT))


def device_rates(chains, reps):
    from powersystemsreliabilityassessment_amd import _abi, _lib, api, case24, hl1
    gens, load = hl1.rts24_generators(), hl1.rts24_load()
    eng = api.Engine(case24.rts24(), device=0)
    hl1._seq_model_load(eng, gens, load)
    start = _abi.HL1_START_STATIONARY

    def seq(seed):
        acc = _abi.Hl1SeqAcc()
        eng._check(eng.L.relmc_hl1_seq(eng._h, seed, 0, chains, 1, start, C.byref(acc), None), "relmc_hl1_seq")
        return eng.last_kernel_ms(), acc

    def storage(seed, st):
        arr = (_abi.Hl1Storage * max(len(st), 1))(*[_abi.Hl1Storage(*s) for s in st])
        acc = _abi.Hl1StorageAcc()
        eng._check(eng.L.relmc_hl1_seq_storage(eng._h, seed, 0, chains, 1, start, 1.0, 0.0, len(st), arr if st else None, C.byref(acc), None, None),
                   "relmc_hl1_seq_storage")
        return eng.last_kernel_ms(), acc

    seq(1)                                                 # warm-up: code objects, buffers
    for _, st in VARIANTS:
        storage(1, st)
    ms = {"relmc_hl1_seq": []}
    ms.update({name: [] for name, _ in VARIANTS})
    accs = {}
    for r in range(reps):
        for name, st in VARIANTS:                          # alternating: every storage timing has a relmc_hl1_seq timing right before it
            ms["relmc_hl1_seq"].append(seq(1 + r)[0])
            t, accs[name] = storage(1 + r, st)
            ms[name].append(t)
    base = statistics.median(ms["relmc_hl1_seq"])
    print(f"{chains} chains x 1 year, stationary, RTS-24; code object {_lib.code_object_sha256()[:12]}; kernel time = relmc_last_kernel_ms", flush=True)
    for name, v in ms.items():
        med = statistics.median(v)
        print(f"  {name:16s} median {med:8.3f} ms  min {min(v):8.3f}  max {max(v):8.3f}  (n = {len(v)})  ratio to relmc_hl1_seq {med / base:.3f}", flush=True)
    for name, a in accs.items():
        print(f"  {name:16s} LOLE {a.sum_lole / a.years:.4f} h/yr  EUE {a.sum_eue / a.years:.2f} MWh/yr  LOLF {a.sum_lolf / a.years:.4f}  "
              f"served {a.sum_served / a.years:.4f} h/yr  discharged {a.sum_discharged / a.years:.2f}  charged {a.sum_charged / a.years:.2f} MWh/yr", flush=True)
    eng.close()


def host_share(chains):
    spec = importlib.util.spec_from_file_location("m", os.path.join(ROOT, "tests", "tools", "hl1_storage_model.py"))
    SM = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(SM)
    from powersystemsreliabilityassessment_amd import hl1
    gens, load = hl1.rts24_generators(), hl1.rts24_load()
    cap = [g.capacity for g in gens]; mf = [g.mttf for g in gens]; mr = [g.mttr for g in gens]
    for name, st in VARIANTS:
        t = time.perf_counter()
        _, c = SM.storage_model(1, range(chains), cap, mf, mr, load.hourly_load, 1, SM.SEQ.STATIONARY, st)
        steps = c["short"] + c["long"] + c["equal"]
        print(f"host model, {name}: {chains} chains, {c['short']} of {steps} steps short, {c['serial_groups']} of {c['groups']} 64-step groups "
              f"take the serial stage ({100.0 * c['serial_groups'] / c['groups']:.2f} %); {time.perf_counter() - t:.1f} s", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=200000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-chains", type=int, default=100)
    a = ap.parse_args()
    device_rates(a.chains, a.reps)
    if a.host_chains > 0:
        host_share(a.host_chains)
