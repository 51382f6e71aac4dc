"""HL1 sequential chronology (relmc_hl1_seq) on RTS-24: simulated years/s and relmc_last_kernel_ms of three shapes, and the host
model's years/s as the CPU point.
  python scripts/hl1_seq_rate.py              every case in a child process of its own under `timeout -k 10`, stops at the first failure
  python scripts/hl1_seq_rate.py --case a     one case in this process (what `rocprofv3 --kernel-trace --stats -- python ... --case a` runs)
Cases: (a) 2e5 chains x 1 year, stationary start; (b) 4096 chains x 25 years, all-UP; (c) 1 chain x 1e4 years, all-UP (the reference's
shape: one wavefront walks the whole chain, latency-bound by design)."""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"a": (200000, 1, "stationary"), "b": (4096, 25, "all_up"), "c": (1, 10000, "all_up")}


def run_case(name):
    from powersystemsreliabilityassessment_amd import _lib, api, case24, hl1
    chains, ypc, start = CASES[name]
    years = chains * ypc
    gens, load = hl1.rts24_generators(), hl1.rts24_load()
    eng = api.Engine(case24.rts24(), device=0)
    hl1.run_sequential_mc(gens, load, years, seed=1, chains=chains, start=start, engine=eng)       # warm-up: code object, buffers
    reps = 5 if name != "c" else 2
    walls, kms = [], []
    for r in range(reps):
        t = time.perf_counter()
        res = hl1.run_sequential_mc(gens, load, years, seed=1 + r, chains=chains, start=start, engine=eng)
        walls.append(time.perf_counter() - t)
        kms.append(eng.last_kernel_ms())
    w, k = min(walls), min(kms)
    print(f"({name}) {chains} chains x {ypc} years, {start}: wall {w * 1e3:.2f} ms ({years / w:.3e} years/s), "
          f"relmc_last_kernel_ms {k:.3f} ({years / (k * 1e-3):.3e} years/s); LOLE {res.lole_hours_yr:.4f} EUE {res.eue_mwh_yr:.2f} "
          f"LOLF {res.lolf_occ_yr:.4f} LOLD {res.lold_hours:.3f}; code object {_lib.code_object_sha256()[:12]}", flush=True)
    eng.close()


def host_rate():
    import importlib.util
    spec = importlib.util.spec_from_file_location("m", os.path.join(ROOT, "tests", "tools", "hl1_seq_model.py"))
    M = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(M)
    from powersystemsreliabilityassessment_amd import hl1
    gens, load = hl1.rts24_generators(), hl1.rts24_load()
    cap = [g.capacity for g in gens]; mf = [g.mttf for g in gens]; mr = [g.mttr for g in gens]
    t = time.perf_counter(); M.interval_model(1, range(64), cap, mf, mr, load.hourly_load, 1, M.STATIONARY); dt = time.perf_counter() - t
    print(f"host model, interval form (numpy, one core): {64 / dt:.1f} years/s", flush=True)
    t = time.perf_counter(); M.literal_chain(1, 0, cap, mf, mr, load.hourly_load, 3, M.ALL_UP); dt = time.perf_counter() - t
    print(f"host model, the reference's hour loop (pure Python, one core): {3 / dt:.2f} years/s", flush=True)


if __name__ == "__main__":
    if "--case" in sys.argv:
        run_case(sys.argv[sys.argv.index("--case") + 1])
        sys.exit(0)
    for name in CASES:
        rc = subprocess.call(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--case", name])
        if rc != 0:
            print(f"case ({name}) ended with status {rc}; no further GPU case is started", flush=True)
            sys.exit(1)
    host_rate()
