"""Loss events of the HL1 sequential chronology (relmc_hl1_seq_events) on hl1_seq_rate.py's shape (a): 2e5 one-year RTS-24 chains,
stationary start.  Three forms, alternated in one process, 5 rounds each after a warm-up round:
  seq        relmc_hl1_seq (no per-year copy)           -- from --seq-lib PATH if given (a build of another revision), else this build
  events     relmc_hl1_seq_events, histogram, no list
  events+list  the same with a list that holds every event (a second walk of the chains)
Prints relmc_last_kernel_ms (min and median) and the wall time of each form, the event count, and both code-object hashes.
  python scripts/hl1_event_rate.py [--seq-lib PATH] [--chains N]"""
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from powersystemsreliabilityassessment_amd import _abi, _lib, hl1  # noqa: E402


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def open_ctx(L, cap, mttf, mttr, load):
    dp = _abi.c_double_p
    L.relmc_ctx_create.argtypes = [C.c_int32, C.POINTER(C.c_void_p)]
    L.relmc_hl1_seq_load.argtypes = [C.c_void_p, C.c_int32, dp, dp, dp, C.c_int32, dp]
    L.relmc_hl1_seq.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int64, C.c_int32, C.c_int32, C.POINTER(_abi.Hl1SeqAcc), C.c_void_p]
    L.relmc_last_kernel_ms.argtypes = [C.c_void_p, dp]
    L.relmc_ctx_destroy.argtypes = [C.c_void_p]
    L.relmc_ctx_destroy.restype = None
    h = C.c_void_p()
    assert L.relmc_ctx_create(0, C.byref(h)) == 0
    assert L.relmc_hl1_seq_load(h, cap.size, cap.ctypes.data_as(dp), mttf.ctypes.data_as(dp), mttr.ctypes.data_as(dp), load.size,
                                load.ctypes.data_as(dp)) == 0
    return h


def kernel_ms(L, h):
    ms = C.c_double()
    L.relmc_last_kernel_ms(h, C.byref(ms))
    return ms.value


if __name__ == "__main__":
    chains = int(arg("--chains", "200000"))
    seq_path = arg("--seq-lib", None)
    gens, lm = hl1.rts24_generators(), hl1.rts24_load()
    cap = np.array([g.capacity for g in gens]); mttf = np.array([g.mttf for g in gens]); mttr = np.array([g.mttr for g in gens])
    load = np.ascontiguousarray(lm.hourly_load, dtype=np.float64)
    L = _lib.load()
    Ls = C.CDLL(seq_path) if seq_path else L
    h, hs = open_ctx(L, cap, mttf, mttr, load), None
    hs = open_ctx(Ls, cap, mttf, mttr, load) if seq_path else h
    ev = np.zeros(8 * chains, dtype=hl1.EVENT_DTYPE)
    hist = np.zeros(168, dtype=np.int64)
    sacc, eacc = _abi.Hl1SeqAcc(), _abi.Hl1EventAcc()

    def seq(seed):
        assert Ls.relmc_hl1_seq(hs, seed, 0, chains, 1, 1, C.byref(sacc), None) == 0
        return kernel_ms(Ls, hs)

    def events(seed, cap_ev):
        assert L.relmc_hl1_seq_events(h, seed, 0, chains, 1, 1, C.byref(eacc), 168, hist.ctypes.data_as(_abi.c_int64_p), cap_ev,
                                      ev.ctypes.data_as(C.POINTER(_abi.Hl1Event))) == 0
        assert cap_ev == 0 or eacc.events <= cap_ev
        return kernel_ms(L, h)

    forms = {"seq": seq, "events": lambda s: events(s, 0), "events+list": lambda s: events(s, ev.size)}
    ms = {k: [] for k in forms}
    wall = {k: [] for k in forms}
    for r in range(6):                                   # round 0 warms up: code objects, buffers
        for k, fn in forms.items():
            t = time.perf_counter()
            m = fn(1 + r)
            if r:
                ms[k].append(m); wall[k].append((time.perf_counter() - t) * 1e3)
        assert eacc.events == sacc.sum_lolf and eacc.sum_dur == sacc.sum_lole, "the two tracks disagree"
    for k in forms:
        print(f"{k:12s} relmc_last_kernel_ms min {min(ms[k]):8.3f} median {statistics.median(ms[k]):8.3f}   wall min {min(wall[k]):8.3f} ms"
              f"   ({chains / (min(ms[k]) * 1e-3):.3e} years/s)", flush=True)
    print(f"{chains} one-year chains, stationary: {eacc.events} events, LOLF {eacc.events / chains:.4f}, LOLD {eacc.sum_dur / eacc.events:.3f} h, "
          f"max duration {eacc.max_dur} h, max energy {eacc.max_energy:.0f} MWh, max peak {eacc.max_peak:.0f} MW")
    print(f"code object {_lib.code_object_sha256()[:12]}" + (f", seq from {_lib.code_object_sha256(seq_path)[:12]}" if seq_path else ""))
    L.relmc_ctx_destroy(h)
    if seq_path:
        Ls.relmc_ctx_destroy(hs)
