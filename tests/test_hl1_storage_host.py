"""Energy storage on the HL1 sequential chronology (relmc_hl1_seq_storage) without a GPU: the host model on a pattern worked out by hand,
its invariants and the paths its fixtures reach, the C ABI's export and struct layouts, and the Python argument checks that need no device."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

from powersystemsreliabilityassessment_amd import _abi, _lib, hl1, hl1_storage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("hl1_storage_model", os.path.join(ROOT, "tests", "tools", "hl1_storage_model.py"))
SM = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(SM)
M = SM.SEQ

# the storages of the two fixtures: (charge_mw, discharge_mw, energy_mwh, eta_charge, eta_discharge, soc0_mwh)
SMALL_STORAGES = [(20.0, 20.0, 60.0, 0.9, 0.95, 60.0), (10.0, 15.0, 30.0, 0.85, 1.0, 0.0)]
F513_STORAGES = [(30.0, 30.0, 90.0, 0.9, 0.9, 90.0), (15.0, 25.0, 40.0, 0.8, 1.0, 0.0), (5.0, 5.0, 1000.0, 1.0, 1.0, 500.0)]


def test_hand_pattern_on_the_model():
    """cap = 100 MW at every step; storage 20 MW / 30 MWh, eta_charge 1.0, eta_discharge 0.5 (a delivered MW costs 2 MWh), full at 30.
    hour  L    step                                                       s after   deficit
    year 1
      0   103  need 3:  avail min(20, 30 * .5 = 15), x 3,  s 30 - 6             24        0   served
      1   110  need 10: avail min(20, 12),           x 10, s 24 - 20            4         0   served
      2   112  need 12: avail min(20, 2),            x 2,  s 4 - 4              0         10  event 1
      3   104  need 4:  avail min(20, 0),            x 0                        0         4
      4   100  cap == L                                                         0         0
      5   96   surplus 4:  room 30, y min(20, 30, 4) = 4                        4         0
      6   101  need 1:  avail min(20, 2),            x 1,  s 4 - 2              2         0   served
      7   60   surplus 40: room 28, y min(20, 28, 40) = 20                      22        0
      8   50   surplus 50: room 8,  y min(20, 8, 50) = 8                        30        0
      9   130  need 30: avail min(20, 15),           x 15, s 30 - 30            0         15  event 2
    year 2 (the state and the open event carry over)
      0   103  need 3:  avail 0                                                 0         3   still event 2: not counted again
      1-3      avail 0                                                          0         10, 12, 4
      4   100  cap == L                                                         0         0
      5-9      as in year 1                                                     4, 2, 22, 30, 0   0, 0, 0, 0, 15  event 3
    year 1: lole 3, eue 29, lolf 2, served 3, discharged 3 + 10 + 2 + 1 + 15 = 31, charged 4 + 20 + 8 = 32
    year 2: lole 5, eue 44, lolf 1, served 1, discharged 1 + 15 = 16, charged 32"""
    curve, storage, soc, deficit, want = SM.hand_pattern()
    trace, cnt = [], SM.new_counters()
    rec, final = SM.storage_chain([100.0] * 20, curve, 2, [storage], cnt, trace)
    assert [t[0][0] for t in trace] == soc
    assert [t[1] for t in trace] == deficit
    np.testing.assert_array_equal(rec, want)
    assert final == [0.0]
    assert (cnt["short"], cnt["long"], cnt["equal"], cnt["served"], cnt["lost"]) == (12, 6, 2, 4, 8)
    # without the storage every short step is a loss step
    base, _ = SM.storage_chain([100.0] * 20, curve, 2, [])
    np.testing.assert_array_equal(base, [[6.0, 60.0, 3.0, 0.0, 0.0, 0.0], [6.0, 60.0, 2.0, 0.0, 0.0, 0.0]])
    np.testing.assert_array_equal(rec[:, 0] + rec[:, 3], base[:, 0])


@pytest.mark.parametrize("start", [M.ALL_UP, M.STATIONARY])
def test_model_served_plus_lole_is_the_base_lole_and_no_storage_is_the_sequential_model(start):
    cap, mttf, mttr, load = M.small_fleet()
    base, _ = SM.storage_model(7, range(8), cap, mttf, mttr, load, 3, start, [])
    L, E, F = M.interval_model(7, range(8), cap, mttf, mttr, load, 3, start)
    np.testing.assert_array_equal(base[:, 0], L)
    np.testing.assert_array_equal(base[:, 2], F)
    np.testing.assert_allclose(base[:, 1], E, rtol=1e-12)
    assert not base[:, 3:].any()
    rec, _ = SM.storage_model(7, range(8), cap, mttf, mttr, load, 3, start, SMALL_STORAGES)
    np.testing.assert_array_equal(rec[:, 0] + rec[:, 3], base[:, 0])
    assert 0 < rec[:, 0].sum() < base[:, 0].sum() and rec[:, 1].sum() < base[:, 1].sum()
    # a storage that cannot discharge, one without energy, and an empty one that cannot charge change nothing
    for idle in ((20.0, 0.0, 60.0, 0.9, 0.95, 60.0), (20.0, 20.0, 0.0, 0.9, 0.95, 0.0), (0.0, 20.0, 60.0, 0.9, 0.95, 0.0)):
        rec, _ = SM.storage_model(7, range(8), cap, mttf, mttr, load, 3, start, [idle, idle])
        np.testing.assert_array_equal(rec[:, :3], base[:, :3])
        assert not rec[:, 3:5].any()


def test_model_is_monotone_in_the_shift_with_one_storage():
    cap, mttf, mttr, load = M.small_fleet()
    rows = [SM.storage_model(7, range(8), cap, mttf, mttr, load, 3, M.STATIONARY, SMALL_STORAGES[:1], shift=s)[0] for s in (-10.0, 0.0, 10.0, 20.0)]
    for a, b in zip(rows, rows[1:]):
        assert (a[:, 0] <= b[:, 0]).all() and (a[:, 1] <= b[:, 1]).all()
    assert rows[0][:, 0].sum() < rows[-1][:, 0].sum()


def test_fixtures_reach_every_path():
    """The two fixtures of tests/test_hl1_storage.py: both branches of every min / max of the step rule are taken, storages run empty and
    fill up again, the second storage is reached, and some groups are quiet while others take the serial stage."""
    cap, mttf, mttr, load = M.small_fleet()
    base, _ = SM.storage_model(7, range(8), cap, mttf, mttr, load, 3, M.STATIONARY, [])
    rec, c = SM.storage_model(7, range(8), cap, mttf, mttr, load, 3, M.STATIONARY, SMALL_STORAGES)
    assert 0 < rec[:, 0].sum() < base[:, 0].sum()
    assert c["empty_after"][0] > 0 and c["discharge"][1] > 0 and c["charge"][0] > 0 and c["charge"][1] > 0
    assert c["clamp"] > 0 and c["served"] > 0 and c["lost"] > 0
    assert 0 < c["serial_groups"] < c["groups"]
    cap, mttf, mttr, load = M.fleet100(513)
    base, _ = SM.storage_model(7, range(4), cap, mttf, mttr, load, 3, M.STATIONARY, [])
    rec, c = SM.storage_model(7, range(4), cap, mttf, mttr, load, 3, M.STATIONARY, F513_STORAGES)
    assert 0 < rec[:, 0].sum() < base[:, 0].sum()
    assert c["clamp"] > 0 and all(c["discharge"][i] > 0 and c["charge"][i] > 0 for i in range(3))
    assert 0 < c["serial_groups"] < c["groups"]


def test_library_exports_the_storage_entry_point():
    hdr = open(os.path.join(ROOT, "include", "relmc.h")).read()
    assert re.search(r"\brelmc_hl1_seq_storage\s*\(", hdr)
    assert "#define RELMC_HL1_MAX_STORAGE 8" in hdr and _abi.HL1_MAX_STORAGE == 8
    assert "relmc_hl1_seq_storage" in _lib.EXPORTS
    assert ":relmc_hl1_seq_storage" in open(os.path.join(ROOT, "julia", "RelMC.jl")).read()
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    assert hasattr(_lib.load(), "relmc_hl1_seq_storage")


def test_storage_struct_layouts_match_the_mirrors(tmp_path):
    """sizeof / offsetof of the three structs from the C compiler == the ctypes mirrors (field names and order included) == the field
    lists of julia/RelMC.jl's structs."""
    pairs = [("relmc_hl1_storage", _abi.Hl1Storage, "Hl1Storage"), ("relmc_hl1_storage_year", _abi.Hl1StorageYear, "Hl1StorageYear"),
             ("relmc_hl1_storage_acc", _abi.Hl1StorageAcc, "Hl1StorageAcc")]
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "relmc.h"', 'int main(void) {']
    for name, m, _ in pairs:
        prog.append(f'printf("%zu", sizeof({name}));')
        prog += [f'printf(" %zu", offsetof({name}, {f}));' for f, _ in m._fields_]
        prog.append('printf("\\n");')
    prog.append('return 0; }')
    src = tmp_path / "layout.c"
    src.write_text("\n".join(prog))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    lines = subprocess.check_output([exe], text=True).splitlines()
    jl = open(os.path.join(ROOT, "julia", "RelMC.jl")).read()
    for (name, m, jname), line in zip(pairs, lines):
        got = [int(x) for x in line.split()]
        assert got == [C.sizeof(m)] + [getattr(m, f).offset for f, _ in m._fields_], name
        body = re.search(r"struct %s\n(.*?)\n(?:    \w+\(\) = new\(\)\n)?end" % jname, jl, re.S).group(1)
        jtypes = {C.c_double: "Cdouble", C.c_int64: "Int64"}
        assert re.findall(r"(\w+)::(\w+)", body) == [(f, jtypes[t]) for f, t in m._fields_], name
    assert [int(x) for x in lines[0].split()][0] == 48 and [int(x) for x in lines[1].split()][0] == 24 and [int(x) for x in lines[2].split()][0] == 104


class _Untouchable:
    """Stands in for the engine: any use of it fails the test."""
    def __getattr__(self, name):
        raise AssertionError(f"the engine was touched ({name}) before the arguments were checked")


def test_storage_arguments_are_checked_before_the_engine():
    gens, load = hl1.rts24_generators(), hl1.rts24_load()
    S = hl1_storage.Storage
    ok = [S(100.0, 100.0, 400.0, 0.92, 0.92)]
    nan, inf = float("nan"), float("inf")
    bad = [dict(years=10, chains=3), dict(years=0), dict(years=10, start="cold"), dict(years=10, scale=nan), dict(years=10, shift=inf),
           dict(years=10, storages=ok * 9), dict(years=10, storages=[S(-1.0, 1.0, 1.0)]), dict(years=10, storages=[S(1.0, -1.0, 1.0)]),
           dict(years=10, storages=[S(1.0, 1.0, -1.0)]), dict(years=10, storages=[S(nan, 1.0, 1.0)]), dict(years=10, storages=[S(1.0, 1.0, inf)]),
           dict(years=10, storages=[S(1.0, 1.0, 1.0, eta_charge=0.0)]), dict(years=10, storages=[S(1.0, 1.0, 1.0, eta_discharge=1.5)]),
           dict(years=10, storages=[S(1.0, 1.0, 1.0, soc0_mwh=2.0)]), dict(years=10, storages=[S(1.0, 1.0, 1.0, soc0_mwh=-0.5)]),
           dict(years=10, storages=ok + [S(1.0, 1.0, 1.0, eta_charge=nan)])]
    for kw in bad:
        with pytest.raises(ValueError):
            hl1_storage.run_sequential_storage(gens, load, **{"storages": ok, "engine": _Untouchable(), **kw})
    with pytest.raises(ValueError, match="eta_charge of storage 1"):
        hl1_storage.run_sequential_storage(gens, load, ok + [S(1.0, 1.0, 1.0, eta_charge=nan)], 10, engine=_Untouchable())
    for kw in (dict(storages=[]), dict(metric="lolf"), dict(bracket=(3.0, 1.0)), dict(rounds=0), dict(start="cold"), dict(chains=3),
               dict(storages=[S(1.0, 1.0, 1.0, eta_discharge=0.0)])):
        with pytest.raises(ValueError):
            hl1_storage.storage_elcc(gens, load, **{"storages": ok, "years": 10, "engine": _Untouchable(), **kw})
    assert S(1.0, 2.0, 3.0).soc0 == 3.0 and S(1.0, 2.0, 3.0, soc0_mwh=0.0).soc0 == 0.0


def test_storage_report():
    base = hl1.SequentialReliabilityResult("Sequential MC", 9.5, 1200.0, 0.1, lolf_occ_yr=2.0)
    st = hl1_storage.StorageReliabilityResult("Sequential MC + storage", 6.25, 900.0, 0.1, lolf_occ_yr=1.5, served_hours_yr=3.25,
                                              discharged_mwh_yr=310.5, charged_mwh_yr=366.25, storages=(hl1_storage.Storage(100.0, 100.0, 400.0),))
    txt = hl1_storage.storage_report(base, st)
    assert "STORAGE SUMMARY" in txt and "9.5000" in txt and "6.2500" in txt and "1 storage:" in txt and "3.2500 short hours/yr" in txt
    assert "310.50 MWh/yr delivered" in txt and "366.25 MWh/yr of surplus taken" in txt
