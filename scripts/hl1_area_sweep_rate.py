"""Multi-area sweep (relmc_hl1_area_sweep): relmc_last_kernel_ms of one 8-level sweep beside the 8 runs of relmc_hl1_area it replaces, on the
same build.
  python scripts/hl1_area_sweep_rate.py              every case in a child process of its own under `timeout -k 10`, stops at the first failure
  python scripts/hl1_area_sweep_rate.py --case rts96 one case in this process
  python scripts/hl1_area_sweep_rate.py --tie-outages   (with or without --case) the same cases with failing ties, as scripts/hl1_area_rate.py
Cases: RTS-96 and the demo system, 2e5 chains x 1 year, stationary start, flow "max_flow".  The 8 levels are a planner's round: tie scales
0, 0.5, 1 and 2 at the loaded curves, and four load shifts in one area at the loaded ties.  The 8 single runs are
run_fast_sequential_simulation(INTERCONNECTED) on level_system(...) of each level: the models the levels are bitwise equivalent to.  Every
figure is the minimum over the repetitions of a call's relmc_last_kernel_ms (chronology kernel and record reductions; no host time)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"rts96": (200000, [100.0, 200.0, 300.0, 400.0]), "demo": (200000, [50.0, 100.0, 150.0, 200.0])}
REPS = 5


def run_case(name, tie_outages=False):
    import numpy as np
    from powersystemsreliabilityassessment_amd import _lib, api, case24, hl1_areas
    chains, shifts = CASES[name]
    sysm = hl1_areas.rts96_system(tie_outages=tie_outages) if name == "rts96" else hl1_areas.demo_system()
    if tie_outages and name == "demo":
        sysm = hl1_areas.System(sysm.areas, [hl1_areas.TieLine(1, 2, 200.0, 950.0, 50.0)])
    n = len(sysm.areas)
    L = hl1_areas.AreaSweepLevel
    levels = [L(tie_scale=s) for s in (0.0, 0.5, 1.0, 2.0)] + [L(load_shift=[v if a == n - 1 else 0.0 for a in range(n)]) for v in shifts]
    eng = api.Engine(case24.rts24(), device=0)
    kw = dict(chains=chains, start="stationary", flow="max_flow", engine=eng)
    hl1_areas.run_area_sweep(sysm, chains, levels, seed=1, **kw)                          # warm-up: code object, buffers
    sweep_ms = []
    for r in range(REPS):
        sw = hl1_areas.run_area_sweep(sysm, chains, levels, seed=1 + r, **kw)
        sweep_ms.append(eng.last_kernel_ms())
    single = []
    for j, lv in enumerate(levels):
        sj = hl1_areas.level_system(sysm, lv)
        hl1_areas.run_fast_sequential_simulation(sj, hl1_areas.INTERCONNECTED, chains, seed=1, **kw)
        ms = []
        for r in range(REPS):
            res = hl1_areas.run_fast_sequential_simulation(sj, hl1_areas.INTERCONNECTED, chains, seed=1 + r, **kw)
            ms.append(eng.last_kernel_ms())
        assert np.array_equal(res.year_indices, sw.year_indices[j]), j                     # the last repetition: same seed, same records
        single.append(min(ms))
    k, tot = min(sweep_ms), sum(single)
    print(f"({name}){' with failing ties' if tie_outages else ''} {chains} chains x 1 year, stationary, max_flow, 8 levels: sweep "
          f"relmc_last_kernel_ms {k:.3f} (median {sorted(sweep_ms)[REPS // 2]:.3f}); 8 runs of relmc_hl1_area {tot:.3f} "
          f"({', '.join('%.3f' % v for v in single)}); ratio {k / tot:.3f}; system LOLE per level "
          f"{', '.join('%.4f' % v for v in sw.lole[:, n])}; code object {_lib.code_object_sha256()[:12]}", flush=True)
    eng.close()


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
