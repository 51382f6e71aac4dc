"""Loss attribution on the HL1 sequential chronology (relmc_hl1_attr_seq) on hl1_seq_rate.py's shape (a): 2e5 one-year RTS-24 chains,
stationary start.  Three forms, alternated in one process, 5 rounds each after a warm-up round:
  seq   (a) relmc_hl1_seq (no per-year copy)
  attr  (b) relmc_hl1_attr_seq at (1.0, 0.0): the same year records, and the unit records summed on the device (none copied back)
  ms    (c) relmc_hl1_ms_seq on the same fleet as two-state units (the track that adds work to every 64-step group)
Prints relmc_last_kernel_ms (min and median) and the wall time of each form, chain-years per second, the ratios b/a, c/a and b/c of the
medians, the two leading units, and the code-object hash.
  python scripts/hl1_attr_rate.py [--chains N]"""
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from powersystemsreliabilityassessment_amd import _abi, _lib, api, case24, hl1, hl1_multistate as ms  # noqa: E402


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


if __name__ == "__main__":
    chains = int(arg("--chains", "200000"))
    gens, load = hl1.rts24_generators(), hl1.rts24_load()
    K = len(gens)
    eng = api.Engine(case24.rts24(), device=0)
    hl1._seq_model_load(eng, gens, load)
    ms._model_load(eng, [ms.MultiStateUnit.from_generator(g) for g in gens], ms._load_array("hl1_attr_rate", load))
    start = _abi.HL1_START_STATIONARY
    sacc, aacc, macc = _abi.Hl1SeqAcc(), _abi.Hl1SeqAcc(), _abi.Hl1MsAcc()
    uacc = (_abi.Hl1AttrAcc * K)()

    def seq(seed):
        eng._check(eng.L.relmc_hl1_seq(eng._h, seed, 0, chains, 1, start, C.byref(sacc), None), "relmc_hl1_seq")
        return eng.last_kernel_ms()

    def attr(seed):
        eng._check(eng.L.relmc_hl1_attr_seq(eng._h, seed, 0, chains, 1, start, 1.0, 0.0, C.byref(aacc), None, uacc, None), "relmc_hl1_attr_seq")
        return eng.last_kernel_ms()

    def multistate(seed):
        eng._check(eng.L.relmc_hl1_ms_seq(eng._h, seed, 0, chains, 1, start, C.byref(macc), None, None), "relmc_hl1_ms_seq")
        return eng.last_kernel_ms()

    forms = {"seq": seq, "attr": attr, "ms": multistate}
    t = {k: [] for k in forms}
    wall = {k: [] for k in forms}
    for r in range(6):                                   # round 0 warms up: code objects, buffers
        for k, fn in forms.items():
            t0 = time.perf_counter()
            m = fn(1 + r)
            if r:
                t[k].append(m); wall[k].append((time.perf_counter() - t0) * 1e3)
        # one chronology, the same year records (the tests compare them bitwise): the counts add exactly; the attribution call takes more
        # launches than relmc_hl1_seq (a chain counts its unit records), so its EUE sums are those numbers added in another order
        for f, _ in _abi.Hl1SeqAcc._fields_:
            assert getattr(macc, f) == getattr(sacc, f), "relmc_hl1_ms_seq disagrees: " + f
            a, b = getattr(aacc, f), getattr(sacc, f)
            assert a == b if "eue" not in f else abs(a - b) <= 1e-12 * abs(b), "relmc_hl1_attr_seq disagrees: " + f
    for k in forms:
        print(f"{k:5s} relmc_last_kernel_ms min {min(t[k]):8.3f} median {statistics.median(t[k]):8.3f}   wall min {min(wall[k]):8.3f} ms"
              f"   {chains / (statistics.median(t[k]) * 1e-3):.3e} chain-years/s", flush=True)
    med = {k: statistics.median(v) for k, v in t.items()}
    print(f"b/a {med['attr'] / med['seq']:.3f}   c/a {med['ms'] / med['seq']:.3f}   b/c {med['attr'] / med['ms']:.3f}")
    imp = [uacc[k].sum[0] / sacc.sum_lole for k in range(K)]
    top = sorted(range(K), key=lambda k: -imp[k])[:2]
    print(f"{chains} one-year chains, stationary; LOLE {sacc.sum_lole / chains:.4f} h/yr; importance of units {top[0]} and {top[1]} "
          f"({gens[top[0]].capacity:.0f} and {gens[top[1]].capacity:.0f} MW): {imp[top[0]]:.4f}, {imp[top[1]]:.4f} (last round's seed)")
    print(f"code object {_lib.code_object_sha256()[:12]}")
    eng.close()
