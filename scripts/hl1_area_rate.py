"""HL1 multi-area chronology (relmc_hl1_area): simulated years/s and relmc_last_kernel_ms of four shapes, and the host model's years/s as
the CPU point.
  python scripts/hl1_area_rate.py              every case in a child process of its own under `timeout -k 10`, stops at the first failure
  python scripts/hl1_area_rate.py --case a     one case in this process (what `rocprofv3 --kernel-trace --stats -- python ... --case a` runs)
  python scripts/hl1_area_rate.py --tie-outages   (with or without --case) the same cases with failing ties: RTS-96 joined by the five lines of
                                               rts96_tie_lines() with their RTS-96 outage data, the demo system's tie at MTTF 950 h / MTTR 50 h
Cases: (a) RTS-96, 2e5 chains x 1 year, stationary, INTERCONNECTED, flow "reference" (deficits are rare); (b) the same under ISOLATED;
(c) the demo system, 2e5 x 1, stationary, INTERCONNECTED (Area_Poor is short in ~38 % of the hours: the solve-heavy case); (d) the demo
system, 1 chain x 1e3 years, all-UP, INTERCONNECTED (the reference's shape: one wavefront walks the whole chain)."""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"a": ("rts96", 200000, 1, "stationary", "INTERCONNECTED"), "b": ("rts96", 200000, 1, "stationary", "ISOLATED"),
         "c": ("demo", 200000, 1, "stationary", "INTERCONNECTED"), "d": ("demo", 1, 1000, "all_up", "INTERCONNECTED")}


def run_case(name, tie_outages=False):
    from powersystemsreliabilityassessment_amd import _lib, api, case24, hl1_areas
    which, chains, ypc, start, pol = CASES[name]
    years = chains * ypc
    sysm = hl1_areas.rts96_system(tie_outages=tie_outages) if which == "rts96" else hl1_areas.demo_system()
    if tie_outages and which == "demo":
        sysm = hl1_areas.System(sysm.areas, [hl1_areas.TieLine(1, 2, 200.0, 950.0, 50.0)])
    policy = getattr(hl1_areas, pol)
    eng = api.Engine(case24.rts24(), device=0)
    hl1_areas.run_fast_sequential_simulation(sysm, policy, years, seed=1, chains=chains, start=start, engine=eng)   # warm-up: code object, buffers
    reps = 5 if name != "d" else 2
    walls, kms = [], []
    for r in range(reps):
        t = time.perf_counter()
        res = hl1_areas.run_fast_sequential_simulation(sysm, policy, years, seed=1 + r, chains=chains, start=start, engine=eng)
        walls.append(time.perf_counter() - t)
        kms.append(eng.last_kernel_ms())
    w, k = min(walls), min(kms)
    rows = ", ".join(f"{r.area} LOLE {r.lole:.4f} EUE {r.eue:.2f}" for r in res.results)
    print(f"({name}) {which}{' with failing ties' if tie_outages else ''} {chains} chains x {ypc} years, {start}, {pol}: wall {w * 1e3:.2f} ms ({years / w:.3e} years/s), "
          f"relmc_last_kernel_ms {k:.3f} ({years / (k * 1e-3):.3e} years/s); {rows}; system LOLE {res.system_lole:.4f} "
          f"LOLF {res.system_lolf:.4f}; code object {_lib.code_object_sha256()[:12]}", flush=True)
    eng.close()


def host_rate():
    import importlib.util
    spec = importlib.util.spec_from_file_location("m", os.path.join(ROOT, "tests", "tools", "hl1_area_model.py"))
    M = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(M)
    from powersystemsreliabilityassessment_amd import hl1_areas
    for which, sysm in (("demo", hl1_areas.demo_system()), ("rts96", hl1_areas.rts96_system())):
        g = [x for a in sysm.areas for x in a.generators]
        args = ([len(a.generators) for a in sysm.areas], [x.capacity for x in g], [x.mttf for x in g], [x.mttr for x in g],
                [a.hourly_load for a in sysm.areas], sysm.topology_matrix)
        t = time.perf_counter(); M.interval_model(1, range(16), *args, 1, M.STATIONARY, M.INTERCONNECTED); dt = time.perf_counter() - t
        print(f"host model (a), {which}, INTERCONNECTED (numpy, one core): {16 / dt:.1f} years/s", flush=True)


if __name__ == "__main__":
    ties = "--tie-outages" in sys.argv
    if "--case" in sys.argv:
        run_case(sys.argv[sys.argv.index("--case") + 1], ties)
        sys.exit(0)
    for name in CASES:
        rc = subprocess.call(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--case", name] +
                             (["--tie-outages"] if ties else []))
        if rc != 0:
            print(f"case ({name}) ended with status {rc}; no further GPU case is started", flush=True)
            sys.exit(1)
    host_rate()
