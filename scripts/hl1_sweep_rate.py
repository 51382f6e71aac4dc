"""Load sweep on the HL1 sequential chronology (relmc_hl1_seq_sweep) on hl1_seq_rate.py's shape (a): 2e5 one-year RTS-24 chains,
stationary start.  Six forms, alternated in one process, 5 rounds each after a warm-up round:
  seq        relmc_hl1_seq (no per-year copy)           -- from --seq-lib PATH if given (a build of another revision), else this build
  sweep-K    relmc_hl1_seq_sweep with K = 1, 4, 8, 16 levels of the whole fleet (shifts spread over -300 .. +300 MW; K = 1: shift 0)
  sweep-15+1 15 shifted levels of the whole fleet and one level of the fleet without unit 21 (the ELCC search's call)
Prints relmc_last_kernel_ms (min and median) and the wall time of each form, level-years per second, the ratio of each sweep to K times
`seq`, and both code-object hashes.  No per-year records are copied back.
  python scripts/hl1_sweep_rate.py [--seq-lib PATH] [--chains N]"""
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


def levels(shifts, withheld_last=False):
    lv = [_abi.Hl1SweepLevel(1.0, float(s), 0, 0) for s in shifts]
    if withheld_last:
        lv.append(_abi.Hl1SweepLevel(1.0, 0.0, 1, 0))
    return (_abi.Hl1SweepLevel * len(lv))(*lv)


if __name__ == "__main__":
    chains = int(arg("--chains", "200000"))
    seq_path = arg("--seq-lib", None)
    gens, lm = hl1.rts24_generators(), hl1.rts24_load()
    cap = np.array([g.capacity for g in gens]); mttf = np.array([g.mttf for g in gens]); mttr = np.array([g.mttr for g in gens])
    load = np.ascontiguousarray(lm.hourly_load, dtype=np.float64)
    L = _lib.load()
    Ls = C.CDLL(seq_path) if seq_path else L
    h = open_ctx(L, cap, mttf, mttr, load)
    hs = open_ctx(Ls, cap, mttf, mttr, load) if seq_path else h
    sacc = _abi.Hl1SeqAcc()
    acc = (_abi.Hl1SeqAcc * 16)()
    mask = (C.c_uint32 * 4)()
    mask[21 >> 5] |= 1 << (21 & 31)
    sets = {"sweep-1": levels([0.0]), "sweep-4": levels(np.linspace(-300, 300, 4)), "sweep-8": levels(np.linspace(-300, 300, 8)),
            "sweep-16": levels(np.linspace(-300, 300, 16)), "sweep-15+1": levels(np.linspace(0, 400, 15), withheld_last=True)}

    def seq(seed):
        assert Ls.relmc_hl1_seq(hs, seed, 0, chains, 1, 1, C.byref(sacc), None) == 0
        return kernel_ms(Ls, hs)

    def sweep(seed, lv):
        assert L.relmc_hl1_seq_sweep(h, seed, 0, chains, 1, 1, len(lv), lv, mask, acc, None) == 0
        return kernel_ms(L, h)

    forms = {"seq": seq}
    forms.update({k: (lambda s, lv=lv: sweep(s, lv)) for k, lv in sets.items()})
    ms = {k: [] for k in forms}
    wall = {k: [] for k in forms}
    for r in range(6):                                   # round 0 warms up: code objects, buffers
        for k, fn in forms.items():
            t = time.perf_counter()
            m = fn(1 + r)
            if r:
                ms[k].append(m); wall[k].append((time.perf_counter() - t) * 1e3)
            if k == "sweep-1":                           # the identity level: relmc_hl1_seq's sums (the records are compared by the tests)
                assert (acc[0].sum_lole, acc[0].sum_lolf) == (sacc.sum_lole, sacc.sum_lolf), "the two tracks disagree"
    base = min(ms["seq"])
    for k in forms:
        n = 1 if k == "seq" else len(sets[k])
        print(f"{k:11s} relmc_last_kernel_ms min {min(ms[k]):8.3f} median {statistics.median(ms[k]):8.3f}   wall min {min(wall[k]):8.3f} ms"
              f"   {n * chains / (min(ms[k]) * 1e-3):.3e} level-years/s   {min(ms[k]) / (n * base):.3f} of {n} x seq", flush=True)
    print(f"{chains} one-year chains, stationary")
    print(f"code object {_lib.code_object_sha256()[:12]}" + (f", seq from {_lib.code_object_sha256(seq_path)[:12]}" if seq_path else ""))
    L.relmc_ctx_destroy(h)
    if seq_path:
        Ls.relmc_ctx_destroy(hs)
