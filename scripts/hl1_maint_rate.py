"""Planned maintenance on the HL1 sequential chronology (relmc_hl1_maint_seq) on hl1_seq_rate.py's shape (a): 2e5 one-year RTS-24 chains,
stationary start.  Five forms, alternated in one process, 5 rounds each after a warm-up round:
  seq         (a) relmc_hl1_seq (no per-year copy)
  maint-empty (b) relmc_hl1_maint_seq with one schedule without windows
  maint-lev   (c) with the RTS-24 levelised schedule (the fleet's maintenance weeks through hl1_planning.schedule_maintenance)
  maint-8     (d) with 8 distinct schedules: the levelised one moved on by 0, 6, .. 42 weeks, wrapping the year's end
  maint-8x1   (e) eight one-schedule calls of those same schedules, each with its relmc_hl1_maint_load (kernel times summed)
Prints relmc_last_kernel_ms (min and median) and the wall time of each form, schedule-years per second, the ratios b/a, c/a and d/e of
the medians, and the code-object hash.  No per-year records are copied back.
  python scripts/hl1_maint_rate.py [--chains N]"""
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from powersystemsreliabilityassessment_amd import _abi, _lib, hl1, hl1_maintenance, hl1_planning  # noqa: E402


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def kernel_ms(L, h):
    ms = C.c_double()
    L.relmc_last_kernel_ms(h, C.byref(ms))
    return ms.value


def windows(schedules):
    flat = [_abi.Hl1MaintWindow(j, w.unit, w.start_hour, w.hours) for j, s in enumerate(schedules) for w in s]
    return (_abi.Hl1MaintWindow * max(len(flat), 1))(*flat), len(flat)


if __name__ == "__main__":
    chains = int(arg("--chains", "200000"))
    gens, lm = hl1.rts24_generators(), hl1.rts24_load()
    cap = np.array([g.capacity for g in gens]); mttf = np.array([g.mttf for g in gens]); mttr = np.array([g.mttr for g in gens])
    load = np.ascontiguousarray(lm.hourly_load, dtype=np.float64)
    H = load.size
    lev = hl1_maintenance.levelised_schedule(gens, lm, [u.maintenance_weeks for u in hl1_planning.rts24_planning_units()])
    eight = [[hl1_maintenance.MaintenanceWindow(w.unit, (w.start_hour + 6 * 168 * j) % H, w.hours) for w in lev] for j in range(8)]
    L = _lib.load()
    dp = _abi.c_double_p
    h = C.c_void_p()
    assert L.relmc_ctx_create(0, C.byref(h)) == 0
    assert L.relmc_hl1_seq_load(h, cap.size, cap.ctypes.data_as(dp), mttf.ctypes.data_as(dp), mttr.ctypes.data_as(dp), H, load.ctypes.data_as(dp)) == 0
    sacc = _abi.Hl1SeqAcc()
    acc = (_abi.Hl1SeqAcc * 8)()
    sums = {}

    def seq(seed):
        assert L.relmc_hl1_seq(h, seed, 0, chains, 1, 1, C.byref(sacc), None) == 0
        return kernel_ms(L, h)

    def maint(seed, schedules, out=acc):
        arr, n = windows(schedules)
        assert L.relmc_hl1_maint_load(h, len(schedules), n, arr if n else None) == 0, L.relmc_last_error(h)
        assert L.relmc_hl1_maint_seq(h, seed, 0, chains, 1, 1, 1.0, 0.0, out, None) == 0, L.relmc_last_error(h)
        return kernel_ms(L, h)

    def one_by_one(seed):
        total, one = 0.0, (_abi.Hl1SeqAcc * 1)()
        for j, s in enumerate(eight):
            total += maint(seed, [s], one)
            sums[j] = (one[0].sum_lole, one[0].sum_eue, one[0].sum_lolf)
        return total

    forms = {"seq": seq, "maint-empty": lambda s: maint(s, [[]]), "maint-lev": lambda s: maint(s, [lev]), "maint-8": lambda s: maint(s, eight),
             "maint-8x1": one_by_one}
    count = {"seq": 1, "maint-empty": 1, "maint-lev": 1, "maint-8": 8, "maint-8x1": 8}
    ms = {k: [] for k in forms}
    wall = {k: [] for k in forms}
    lole = {}
    for r in range(6):                                   # round 0 warms up: code objects, buffers
        for k, fn in forms.items():
            t = time.perf_counter()
            m = fn(1 + r)
            if r:
                ms[k].append(m); wall[k].append((time.perf_counter() - t) * 1e3)
            if k == "maint-empty":                       # the empty schedule: relmc_hl1_seq's sums (the records are compared by the tests)
                assert (acc[0].sum_lole, acc[0].sum_eue, acc[0].sum_lolf) == (sacc.sum_lole, sacc.sum_eue, sacc.sum_lolf), "the two tracks disagree"
            if k == "maint-lev":
                lole["lev"] = acc[0].sum_lole / chains
                lole["none"] = sacc.sum_lole / chains
            if k == "maint-8":
                eight_sums = [(acc[j].sum_lole, acc[j].sum_eue, acc[j].sum_lolf) for j in range(8)]
            if k == "maint-8x1":                         # one call of eight == eight calls of one
                assert eight_sums == [sums[j] for j in range(8)], "a schedule's sums depend on its neighbours"
    for k in forms:
        n = count[k]
        print(f"{k:11s} relmc_last_kernel_ms min {min(ms[k]):8.3f} median {statistics.median(ms[k]):8.3f}   wall min {min(wall[k]):8.3f} ms"
              f"   {n * chains / (statistics.median(ms[k]) * 1e-3):.3e} schedule-years/s", flush=True)
    med = {k: statistics.median(v) for k, v in ms.items()}
    print(f"b/a {med['maint-empty'] / med['seq']:.3f}   c/a {med['maint-lev'] / med['seq']:.3f}   d/e {med['maint-8'] / med['maint-8x1']:.3f}   "
          f"d/(8 a) {med['maint-8'] / (8 * med['seq']):.3f}")
    print(f"{chains} one-year chains, stationary; LOLE without maintenance {lole['none']:.4f} h/yr, levelised schedule {lole['lev']:.4f} h/yr (last round's seed)")
    print(f"code object {_lib.code_object_sha256()[:12]}")
    L.relmc_ctx_destroy(h)
