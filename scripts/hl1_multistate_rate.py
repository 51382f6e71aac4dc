"""Three-state units on the HL1 sequential chronology (relmc_hl1_ms_seq) on RTS-24 against relmc_hl1_seq, on hl1_seq_rate.py's shape
(a): 2e5 one-year chains, stationary start.  One process: after a warm-up of every form, each is timed REPS times, the three forms
alternated; kernel time is relmc_last_kernel_ms and the best of the REPS is reported.
  (a) relmc_hl1_seq                                   the two-state kernel
  (b) relmc_hl1_ms_seq, the same fleet as two-state units   (its year records are (a)'s bit for bit: checked here on the sums)
  (c) relmc_hl1_ms_seq, hl1_multistate.derated_rts24()      the 350 MW and 400 MW units with a derated state
Prints the three times, the ratios of (b) and (c) to (a) and the code-object hash.
  python scripts/hl1_multistate_rate.py [--chains N] [--reps R]"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=200000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    from powersystemsreliabilityassessment_amd import _abi, _lib, api, case24, hl1, hl1_multistate as ms
    gens, load = hl1.rts24_generators(), hl1.rts24_load()
    eng = api.Engine(case24.rts24(), device=0)
    hl1._seq_model_load(eng, gens, load)
    hl = ms._load_array("hl1_multistate_rate", load)
    start = _abi.HL1_START_STATIONARY
    fleets = {"b": [ms.MultiStateUnit.from_generator(g) for g in gens], "c": ms.derated_rts24()}

    def seq(seed):
        acc = _abi.Hl1SeqAcc()
        eng._check(eng.L.relmc_hl1_seq(eng._h, seed, 0, a.chains, 1, start, C.byref(acc), None), "relmc_hl1_seq")
        return eng.last_kernel_ms(), acc

    def multistate(seed, which):
        ms._model_load(eng, fleets[which], hl)               # a host-to-device copy of 10 KB when the fleet changes; not in the kernel time
        acc = _abi.Hl1MsAcc()
        eng._check(eng.L.relmc_hl1_ms_seq(eng._h, seed, 0, a.chains, 1, start, C.byref(acc), None, None), "relmc_hl1_ms_seq")
        return eng.last_kernel_ms(), acc

    forms = (("a", "relmc_hl1_seq", lambda s: seq(s)), ("b", "relmc_hl1_ms_seq, two-state fleet", lambda s: multistate(s, "b")),
             ("c", "relmc_hl1_ms_seq, derated_rts24()", lambda s: multistate(s, "c")))
    for _, _, fn in forms:                                   # warm-up: code objects, buffers
        fn(1)
    t = {k: [] for k, _, _ in forms}
    accs = {}
    for r in range(a.reps):
        for k, _, fn in forms:
            ms_, accs[k] = fn(1 + r)
            t[k].append(ms_)
    same = all(getattr(accs["a"], f) == getattr(accs["b"], f) for f, _ in _abi.Hl1SeqAcc._fields_)
    print(f"{a.chains} chains x 1 year, stationary, RTS-24; code object {_lib.code_object_sha256()[:12]}; kernel time = relmc_last_kernel_ms, best of {a.reps}", flush=True)
    base = min(t["a"])
    for k, name, _ in forms:
        x = accs[k]
        extra = "" if k == "a" else f"  derated {x.sum_derated / x.years:.1f}  down {x.sum_down / x.years:.1f} unit-h/yr"
        print(f"  ({k}) {name:36s} best {min(t[k]):8.3f} ms  median {sorted(t[k])[len(t[k]) // 2]:8.3f}  max {max(t[k]):8.3f}  ratio to (a) {min(t[k]) / base:.3f}"
              f"  LOLE {x.sum_lole / x.years:.4f} h/yr  EUE {x.sum_eue / x.years:.2f} MWh/yr  LOLF {x.sum_lolf / x.years:.4f}{extra}", flush=True)
    print(f"  the sums of (b) are {'bitwise those' if same else 'NOT those'} of (a)", flush=True)
    eng.close()
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
