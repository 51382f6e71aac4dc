"""HL1 planning Monte Carlo (relmc_hl1_plan): simulated years/s and relmc_last_kernel_ms of the toy fleet (6 units, 1 ELU, 8760 hours)
and RTS-24 (32 units with their maintenance weeks, 8736 hours) at 1e5 and 1e6 years, then the host model's years/s as the CPU point.
  python scripts/hl1_plan_rate.py              every case in a child process of its own under `timeout -k 10`, stops at the first failure
  python scripts/hl1_plan_rate.py --case toy5  one case in this process (what `rocprofv3 --kernel-trace --stats -- python ... --case toy5` runs)
The last case prints the toy fleet's comparison report (the reference's 2000 years) and its tail summary."""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"toy5": ("toy", 100000), "toy6": ("toy", 1000000), "rts5": ("rts24", 100000), "rts6": ("rts24", 1000000), "report": ("toy", 2000)}


def fleet(name):
    from powersystemsreliabilityassessment_amd import hl1, hl1_planning as P
    if name == "toy":
        units, load = P.toy_fleet(), P.toy_load(1)
    else:
        units, load = P.rts24_planning_units(), hl1.rts24_load().hourly_load
    P.schedule_maintenance(units, P.weekly_peaks(load))
    return units, load


def run_case(name):
    from powersystemsreliabilityassessment_amd import _lib, api, case24, hl1_planning as P
    fl, years = CASES[name]
    units, load = fleet(fl)
    eng = api.Engine(case24.rts24(), device=0)
    if name == "report":
        ana = P.run_detailed_analytical(units, load, 5.0)
        mc = P.run_monte_carlo_simulation(units, load, 5.0, years, seed=1, engine=eng)
        print(P.comparison_report(ana, mc), P.tail_summary(mc.year_lole), flush=True)
        eng.close()
        return
    P.run_monte_carlo_simulation(units, load, 5.0, years, seed=1, engine=eng)         # warm-up: code object, buffers
    walls, kms = [], []
    for r in range(3):
        t = time.perf_counter()
        res = P.run_monte_carlo_simulation(units, load, 5.0, years, seed=2 + r, engine=eng)
        walls.append(time.perf_counter() - t)
        kms.append(eng.last_kernel_ms())
    w, k = min(walls), min(kms)
    print(f"({name}) {fl}, {years} years, 5 % LFU: wall {w * 1e3:.1f} ms ({years / w:.3e} years/s), relmc_last_kernel_ms {k:.2f} "
          f"({years / (k * 1e-3):.3e} years/s); LOLE {res.lole_hours_yr:.4f} EUE {res.eue_mwh_yr:.2f} LOLF {res.lolf_occ_yr:.4f}; "
          f"code object {_lib.code_object_sha256()[:12]}", flush=True)
    eng.close()


def host_rate():
    import importlib.util
    spec = importlib.util.spec_from_file_location("m", os.path.join(ROOT, "tests", "tools", "hl1_plan_model.py"))
    M = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(M)
    for fl in ("toy", "rts24"):
        units, load = fleet(fl)
        arr = ([u.capacity for u in units], [u.for_rate for u in units], [u.scheduled_outage_start for u in units],
               [u.maintenance_weeks for u in units], [u.energy_limit for u in units])
        t = time.perf_counter(); M.model(1, range(64), *arr, load, 0.05 * float(load.max())); dt = time.perf_counter() - t
        print(f"host model ({fl}, numpy, one core): {64 / dt:.1f} years/s", flush=True)


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
