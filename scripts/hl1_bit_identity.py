"""Are the outputs of the eleven HL1 chronology entry points (relmc_hl1_seq, _seq_events, _seq_sweep, _seq_storage, _var_seq, _stress_seq,
_ms_seq, _area, _area_sweep, _area_var, _plan) the same bytes under two builds of the library?  sha256 of every output (acc, the year
records, the second rows, the weather_host arrays, the plan's hour counts and ELU energies, the events' histogram and list) on a one-launch
shape (a) and on a two-launch shape (b: that of each driver's own test; 2100 x 1000 for _var_seq and _stress_seq, 700 x 1000 on two areas
for _area_var, whose launch holds 2^22 / (1000 * 6) = 699 chains), both start rules, both weather picks where the call has one; one fresh
child process per library (RELMC_LIB_PATH), every child under a time limit, then the comparison.  The calls are the raw-ABI helpers of the
tests.
  python scripts/hl1_bit_identity.py PARENT.so [NEW.so] [--out DIR]     -> DIR/bit_identity.txt (default DIR: a new temporary directory, printed), exit 1 if any differ
NEW.so defaults to this tree's build.  Used for profiles/hl1_host_driver/bit_identity.txt, profiles/hl1_storage_devfn/bit_identity.txt, profiles/hl1_storage_template/bit_identity.txt and
profiles/hl1_chain_template/bit_identity.txt."""
import ctypes as C
import hashlib
import importlib.util
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ARGV = [a for a in sys.argv[1:]]
OUT = os.path.abspath(ARGV.pop(ARGV.index("--out") + 1)) if "--out" in ARGV else tempfile.mkdtemp(prefix="hl1_bit_identity_")
ARGV = [a for a in ARGV if a != "--out"]


def _mod(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def child(tag):
    import numpy as np
    from powersystemsreliabilityassessment_amd import _abi, _lib, api, case24, hl1_areas
    TE, TC, TM, TA = _mod("test_hl1_edges"), _mod("test_hl1_chrono_edges"), _mod("test_hl1_multistate"), _mod("test_hl1_area_sweep")
    TS, TV = _mod("test_hl1_stress"), _mod("test_hl1_area_variable")
    E, MM = TE.E, TM.MM
    eng = api.Engine(case24.rts24(), device=0)
    lines = []

    def put(name, *objs):
        h = hashlib.sha256()
        n = 0
        for o in objs:
            b = o.tobytes() if hasattr(o, "tobytes") else bytes(o)
            h.update(b); n += len(b)
        lines.append(f"{name} {n} {h.hexdigest()[:32]}")
        print(lines[-1], flush=True)

    def seq_family(shape, N, Y, levels, wh, st, sweep_shape=None, storage_n=None):
        for start in (0, 1):
            t = f"{shape} start{start}"
            acc, yr = TC._seq(eng, 8, 0, N, Y, start)
            put(f"{t} relmc_hl1_seq acc", acc); put(f"{t} relmc_hl1_seq years_host", yr)
            acc, yr = TC._sweep(eng, 8, 0, *(sweep_shape or (N, Y)), start, levels, wh)
            put(f"{t} relmc_hl1_seq_sweep acc", acc); put(f"{t} relmc_hl1_seq_sweep years_host", yr)
            acc, yr, sy = TC._storage(eng, 8, 0, storage_n or N, Y, start, st)
            put(f"{t} relmc_hl1_seq_storage acc", acc); put(f"{t} relmc_hl1_seq_storage years_host", yr); put(f"{t} relmc_hl1_seq_storage storage_years_host", sy)
            cnt, _, _ = TC._events(eng, 8, 0, N, Y, start, 0)
            acc, hist, ev = TC._events(eng, 8, 0, N, Y, start, max(int(cnt.events), 1))
            put(f"{t} relmc_hl1_seq_events acc", acc); put(f"{t} relmc_hl1_seq_events dur_hist", hist); put(f"{t} relmc_hl1_seq_events list", np.ascontiguousarray(ev))

    def weather_family(shape, N, Y, load, st, mult, cls):
        """relmc_hl1_var_seq and relmc_hl1_stress_seq on the fleet loaded by seq_family: 3 weather years with load curves, 2 resources"""
        out, wl = TS._weather(load, 3, 2, 23, True)
        TS._var_load(eng, out, wl)
        TS._stress_load(eng, mult, cls)
        for fn, run in (("relmc_hl1_var_seq", TS._var), ("relmc_hl1_stress_seq", TS._stress)):
            for start in (0, 1):
                for pick in (TS.RANDOM, TS.CYCLE):
                    t = f"{shape} start{start} pick{pick} {fn}"
                    acc, yr, sy, wy, _ = run(eng, 8, 0, N, Y, start, st, (1.0, 0.5), 1.02, -1.5, pick)
                    put(f"{t} acc", acc); put(f"{t} years_host", yr); put(f"{t} storage_years_host", sy); put(f"{t} weather_host", wy)

    def area_var(shape, N, Y, outages):
        """relmc_hl1_area_var on the 2-area shape of its test (3 rows, 2 resources, 2 storages); with outages the tie-outage kernel"""
        sh, _, _ = TV._setup(eng, "a2", True, outages=outages)
        for start in (0, 1):
            for pick in (TV.RANDOM, TV.CYCLE):
                t = f"{shape} start{start} pick{pick} relmc_hl1_area_var"
                o = TV._opts(rs=sh["resource_scale"], lsc=(1.03, 0.98), lsh=(-2.0, 1.0), flow=TV.MAXF, pick=pick)
                acc, yr, sy, wy, _ = TV._run(eng, 3, 8, 0, N, Y, start, o, sh["storages"])
                put(f"{t} acc", acc); put(f"{t} years_host", yr); put(f"{t} storage_years_host", sy); put(f"{t} weather_host", wy)

    def ms(shape, N, Y):
        for start in (0, 1):
            acc, yr, sy, _ = TM._ms(eng, 8, 0, N, Y, start)
            put(f"{shape} start{start} relmc_hl1_ms_seq acc", acc); put(f"{shape} start{start} relmc_hl1_ms_seq years_host", yr)
            put(f"{shape} start{start} relmc_hl1_ms_seq state_years_host", sy)

    def area(shape, N, Y, rows):
        for start in (0, 1):
            acc, yr = TE._area(eng, rows, 6, 0, N, Y, start, TE.AREA.INTERCONNECTED, TE.AREA.MAX_FLOW)
            put(f"{shape} start{start} relmc_hl1_area acc", acc); put(f"{shape} start{start} relmc_hl1_area years_host", yr)

    def area_sweep(shape, N, Y, rows, levels):
        for start in (0, 1):
            acc, yr = TA._sweep(eng, rows, 6, 0, N, Y, start, TA.SM.MAX_FLOW, levels)
            put(f"{shape} start{start} relmc_hl1_area_sweep acc", acc); put(f"{shape} start{start} relmc_hl1_area_sweep years_host", yr)

    def plan(shape, N, nhours, n_elu):
        acc, yr, hours, elu = TE._plan(eng, 4, 0, N, nhours, n_elu)
        put(f"{shape} relmc_hl1_plan acc", acc); put(f"{shape} relmc_hl1_plan years_host", yr)
        put(f"{shape} relmc_hl1_plan hour_loss_count", hours); put(f"{shape} relmc_hl1_plan elu_energy", np.ascontiguousarray(elu))

    # ---- shape (a): 3 units, a 24-hour curve, 5 chains x 2 years; areas: 2 areas, 1 tie; sweeps: 2 levels
    cap, mttf, mttr, load = E.seq_fleet(3, 24)
    TC._load(eng, cap, mttf, mttr, load)
    seq_family("a", 5, 2, E.edge_levels(2), E.edge_withheld(3), E.edge_storages(cap))
    weather_family("a", 5, 2, load, E.edge_storages(cap), TS.XM.varying_multipliers(3, 2, 24, 17), [0, 1, -1])
    units3 = MM.six_unit_fleet()[0][:3]
    TM._ms_load(eng, units3, MM.six_unit_fleet()[1][:24])
    ms("a", 5, 2)
    eng._check(TE._area_load(eng.L, eng._h, [2, 1], cap, mttf, mttr, np.stack([load * 0.6, load * 0.4]), [(0, 1, 20.0)]), "relmc_hl1_area_load")
    area("a", 5, 2, 3)
    area_sweep("a", 5, 2, 3, [(1.0, 0.0, 1.0, 0), (1.05, 2.0, 0.5, 0)])
    area_var("a", 5, 2, False)
    data, sigma = E.plan_fleet(3, nhours=24, n_elu=1)
    eng._check(TE._plan_load(eng.L, eng._h, data, sigma), "relmc_hl1_plan_load")
    plan("a", 10, 24, 1)

    # ---- shape (b): the two-launch shape of each driver's own test
    cap, mttf, mttr, load = E.seq_fleet(6, 24)
    TC._load(eng, cap, mttf, mttr, load)
    seq_family("b", 4300, 1000, E.edge_levels(16), E.edge_withheld(6), E.edge_storages(cap), sweep_shape=(4100, 64), storage_n=2100)
    weather_family("b", 2100, 1000, load, E.edge_storages(cap), TS.XM.varying_multipliers(3, 2, 24, 17), TS.SIX_CLASSES)
    units, mload = MM.six_unit_fleet()
    TM._ms_load(eng, units, mload[:24])
    ms("b", 2100, 1000)
    cap, mttf, mttr, load = E.seq_fleet(12, 24)
    eng._check(TE._area_load(eng.L, eng._h, [5, 7], cap, mttf, mttr, np.stack([load * 0.45, load * 0.55]), [(0, 1, 20.0)]), "relmc_hl1_area_load")
    area("b", 4300, 1000, 3)
    TA._load(eng, *TA._arrays(hl1_areas.demo_system(hours=24)))
    area_sweep("b", 2800, 64, 3, [(1.0, 10.0 * k, 0.25 * k, 0) for k in range(8)])
    area_var("b", 700, 1000, True)
    data, sigma = E.plan_fleet(6, nhours=24, n_elu=1)
    eng._check(TE._plan_load(eng.L, eng._h, data, sigma), "relmc_hl1_plan_load")
    plan("b", (1 << 20) + 100, 24, 1)
    eng.close()
    with open(os.path.join(OUT, f"digests_{tag}.txt"), "w") as f:
        f.write(f"# {tag}: {os.path.basename(_lib.LIB_PATH)}, .hip_fatbin sha256 {_lib.code_object_sha256()[:16]}\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    if "--child" in ARGV:
        child(ARGV[ARGV.index("--child") + 1])
        sys.exit(0)
    if not ARGV:
        sys.exit(__doc__)
    LIBS = {"parent": os.path.abspath(ARGV[0]),
            "new": os.path.abspath(ARGV[1]) if len(ARGV) > 1 else os.path.join(ROOT, "powersystemsreliabilityassessment_amd", "csrc", "librelmc.so")}
    for tag, lib in LIBS.items():
        rc = subprocess.call(["timeout", "-k", "10", "420", sys.executable, os.path.abspath(__file__), "--child", tag, "--out", OUT],
                             env=dict(os.environ, RELMC_LIB_PATH=lib))
        if rc != 0:
            print(f"child {tag} ended with status {rc}; nothing more is started", flush=True)
            sys.exit(1)
    rows = {}
    heads = []
    for tag in LIBS:
        for ln in open(os.path.join(OUT, f"digests_{tag}.txt")):
            if ln.startswith("#"):
                heads.append(ln.strip()); continue
            name, n, d = ln.rsplit(" ", 2)
            rows.setdefault(name, {})[tag] = (n, d.strip())
    bad = 0
    with open(os.path.join(OUT, "bit_identity.txt"), "w") as f:
        f.write("\n".join(heads) + "\n# output, bytes, sha256[:32] parent, sha256[:32] new\n")
        for name, v in rows.items():
            same = v.get("parent") == v.get("new")
            bad += not same
            f.write(f"{name} {v['parent'][0]} {v['parent'][1]} {v.get('new', ('', 'missing'))[1]} {'identical' if same else 'DIFFERENT'}\n")
        f.write(f"{len(rows)} outputs, {bad} different\n")
    print(open(os.path.join(OUT, "bit_identity.txt")).read()[-400:] + "written to " + OUT)
    sys.exit(1 if bad else 0)
