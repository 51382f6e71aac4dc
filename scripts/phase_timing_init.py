"""Setup shares of one scenario group (-DRELMC_PHASE_TIMING -DRELMC_PT_INIT build passed with RELMC_LIB_PATH).

  python scripts/phase_timing_init.py [nsq24 | rts96 | seq]      (default nsq24)
nsq24: the fused 16-lane kernel, four scenarios per group; rts96: the 64-lane tile, one scenario per group; seq: the sequential
instantiation (MODE 2) on RTS-24 over 25 years' contingency hours, four scenarios per group.  The counters are those of the last launch."""
import os, sys, ctypes as C
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from powersystemsreliabilityassessment_amd import api, case96
workload = sys.argv[1] if len(sys.argv) > 1 else "nsq24"
if workload == "rts96":
    eng = api.Engine(case96.rts96())
    eng.nsq_accumulate(1, 0, 65536)
    acc = eng.nsq_accumulate(1, 1000000, 1000000)
    per_group = 1
elif workload == "seq":
    from powersystemsreliabilityassessment_amd import seq as rseq
    eng = api.Engine()
    sq = rseq.SeqEngine(eng)
    sq.seq_years(1, 0, 25)
    acc = sq.seq_years(1, 25, 25)[4]
    per_group = 4
else:
    eng = api.Engine()
    eng.nsq_accumulate(1, 0, 65536)
    acc = eng.nsq_accumulate(1, 1000000, 1000000)
    per_group = 4
out = (C.c_ulonglong * 8)()
eng.L.relmc_debug_phase_cycles.argtypes = [C.c_void_p, C.POINTER(C.c_ulonglong)]
eng.L.relmc_debug_phase_cycles(eng._h, out)
names = ["window sampling", "state from window", "status -> model", "topology", "susceptance entries", "start point", "interior-point loop", "output"]
tot = sum(out)
print("workload", workload, "scenarios", int(acc.n), "kernel_ms", eng.last_kernel_ms())
for n, v in zip(names, out):
    print(f"{n:22s} {v/tot*100:6.2f} %   {v/(acc.n/per_group):10.1f} cycles per scenario group")
print(f"{'setup (parts 0-5)':22s} {sum(out[:6])/tot*100:6.2f} %   {sum(out[:6])/(acc.n/per_group):10.1f} cycles per scenario group")
