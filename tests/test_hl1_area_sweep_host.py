"""Sweep of the HL1 multi-area chronology (relmc_hl1_area_sweep) without a GPU: the level struct's layout against the C compiler, ctypes
and the Julia table, the export, the host model against the reference's literal loop on a transformed level, the first-crossing rule of
the searches, the report, and the Python argument checks that need no device."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

from powersystemsreliabilityassessment_amd import _abi, _lib, hl1, hl1_areas

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("hl1_area_sweep_model", os.path.join(ROOT, "tests", "tools", "hl1_area_sweep_model.py"))
SM = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(SM)
AM = SM.AM


def test_level_layout_matches_the_mirrors(tmp_path):
    """sizeof / offsetof of relmc_hl1_area_level and the level limit from the C compiler == the ctypes mirror == julia's
    LAYOUT_HL1_AREA_SWEEP and its struct."""
    jl = open(os.path.join(ROOT, "julia", "RelMC.jl")).read()
    block = jl[jl.index("const LAYOUT_HL1_AREA_SWEEP = ["):]
    block = block[:block.index("\n]\n") + 3]
    table = [(m.group(1), int(m.group(2)), [(f, int(o)) for f, o in re.findall(r'\("(\w+)",\s*(\d+)\)', m.group(3))])
             for m in re.finditer(r'\("(relmc_\w+)",\s*(\d+),\s*\[(.*?)\]\)', block)]
    assert [t[0] for t in table] == ["relmc_hl1_area_level"]
    name, size, fields = table[0]
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "relmc.h"', 'int main(void) {',
            'printf("%d %d", (int)RELMC_HL1_AREA_SWEEP_MAX_LEVELS, (int)RELMC_AREA_MAX);', f'printf(" %zu", sizeof({name}));']
    prog += [f'printf(" %zu", offsetof({name}, {f}));' for f, _ in fields]
    prog.append('printf("\\n"); return 0; }')
    src = tmp_path / "layout.c"
    src.write_text("\n".join(prog))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    assert got[:2] == [8, 8] and _abi.HL1_AREA_SWEEP_MAX_LEVELS == 8
    assert int(re.search(r"const HL1_AREA_SWEEP_MAX_LEVELS = (\d+)", jl).group(1)) == 8
    got = got[2:]
    m = _abi.Hl1AreaLevel
    assert got == [size] + [o for _, o in fields] == [144, 0, 64, 128, 136, 140]
    assert got == [C.sizeof(m)] + [getattr(m, f).offset for f, _ in m._fields_]
    assert [f for f, _ in fields] == [f for f, _ in m._fields_]
    body = re.search(r"struct Hl1AreaLevel\n(.*?)\nend", jl, re.S).group(1)
    assert re.findall(r"(\w+)::([\w{},]+)", body) == [("load_scale", "NTuple{8,Cdouble}"), ("load_shift", "NTuple{8,Cdouble}"),
                                                    ("tie_scale", "Cdouble"), ("fleet", "Int32"), ("reserved", "Int32")]
    assert ":relmc_hl1_area_sweep" in jl


def test_library_exports_the_entry_point():
    hdr = open(os.path.join(ROOT, "include", "relmc.h")).read()
    assert re.search(r"\bint32_t relmc_hl1_area_sweep\s*\(relmc_ctx\* ctx, uint64_t seed, uint64_t first_chain, int64_t n_chains", hdr)
    assert "relmc_hl1_area_sweep" in _lib.EXPORTS
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    assert hasattr(_lib.load(), "relmc_hl1_area_sweep")


def _small_system():
    """Three areas of 2 + 3 + 2 units, a 120-hour year, three ties (a triangle), loads near the expected capacities."""
    cap = np.array([30.0, 45.0, 25.0, 20.0, 35.0, 50.0, 40.0])
    mttf = np.array([90.0, 120.0, 70.0, 100.0, 80.0, 110.0, 95.0])
    mttr = np.array([12.0, 9.0, 15.0, 10.0, 14.0, 8.0, 11.0])
    h = np.arange(120)
    loads = np.stack([55.0 + 10.0 * np.sin(2 * np.pi * h / 24.0), 60.0 + 12.0 * np.sin(2 * np.pi * (h - 7) / 24.0),
                      70.0 + 9.0 * np.sin(2 * np.pi * (h + 5) / 24.0)])
    ties = [(0, 1, 12.5), (1, 2, 8.0), (0, 2, 5.25)]
    return [2, 3, 2], cap, mttf, mttr, loads, ties


def test_host_model_equals_the_literal_loop_on_a_transformed_level():
    """One level with per-area scales and shifts, scaled ties of which one keeps its capacity, and a withheld unit: the interval model of
    the sweep equals the reference's hour loop run on the transformed system (integers exactly, EUE to 1e-9), both start rules."""
    units, cap, mttf, mttr, loads, ties = _small_system()
    level = ([1.05, 0.95, 1.0], [2.5, 0.0, -4.0], 0.5, 1)
    c_j, ld_j, ties_j = SM.transform(cap, loads, ties, level, withheld=[3], tie_scaled=[1, 0, 1])
    assert c_j.tolist() == [30.0, 45.0, 25.0, 0.0, 35.0, 50.0, 40.0] and [t[2] for t in ties_j] == [6.25, 8.0, 2.625]
    np.testing.assert_array_equal(ld_j[0], 1.05 * loads[0] + 2.5)
    for start in (SM.ALL_UP, SM.STATIONARY):
        got = SM.sweep_model(7, [4, 5], units, cap, mttf, mttr, loads, ties, None, None, 3, start, SM.REFERENCE, [(1.0, 0.0, 1.0, 0), level],
                             withheld=[3], tie_scaled=[1, 0, 1])
        assert got.shape == (2, 6, 4, 3)
        for q, chain in enumerate((4, 5)):
            want = AM.literal_chain(7, chain, units, c_j, mttf, mttr, ld_j, AM.topology(3, ties_j), 3, start, SM.INTERCONNECTED)
            lvl = got[1, 3 * q:3 * q + 3]
            np.testing.assert_array_equal(lvl[..., 0], want[..., 0])
            np.testing.assert_array_equal(lvl[..., 2], want[..., 2])
            np.testing.assert_allclose(lvl[..., 1], want[..., 1], rtol=1e-9, atol=1e-9)
        assert got[1, :, 3, 0].sum() > got[0, :, 3, 0].sum() > 0                      # the level is the harder one, and both lose load
    # tie scale 0 on every tie = ISOLATED
    zero = SM.sweep_model(7, [4], units, cap, mttf, mttr, loads, ties, None, None, 3, SM.ALL_UP, SM.MAX_FLOW, [(1.0, 0.0, 0.0, 0)])[0]
    iso = AM.interval_model(7, [4], units, cap, mttf, mttr, loads, AM.topology(3, ties), 3, SM.ALL_UP, SM.ISOLATED)
    np.testing.assert_array_equal(zero, iso)


def test_level_system_is_the_transformed_model():
    d = hl1_areas.demo_system(hours=48)
    sysm = hl1_areas.System(d.areas, [hl1_areas.TieLine(1, 2, 200.0, 950.0, 50.0), hl1_areas.TieLine(2, 1, 30.0)])
    lv = hl1_areas.AreaSweepLevel(load_scale=[1.0, 1.1], load_shift=5.0, tie_scale=0.25, withheld=True)
    s = hl1_areas.level_system(sysm, lv, withheld_units=[1, 9], scaled_ties=[0])
    assert [g.capacity for a in s.areas for g in a.generators] == [400.0, 0.0, 400.0, 400.0, 400.0, 200.0, 200.0, 200.0, 200.0, 0.0]
    assert [(t.capacity, t.mttf, t.mttr) for t in s.tie_lines] == [(50.0, 950.0, 50.0), (30.0, np.inf, np.inf)]
    np.testing.assert_array_equal(s.areas[1].hourly_load, 1.1 * np.asarray(d.areas[1].hourly_load) + 5.0)
    np.testing.assert_array_equal(s.areas[0].hourly_load, 1.0 * np.asarray(d.areas[0].hourly_load) + 5.0)
    same = hl1_areas.level_system(sysm, hl1_areas.AreaSweepLevel())
    assert np.array_equal(same.topology_matrix, sysm.topology_matrix) and same.areas[0].generators[1].capacity == 400.0
    assert sysm.areas[0].generators[1].capacity == 400.0                              # the system itself is untouched


def test_first_crossing_on_a_curve_that_is_not_monotone():
    """An area's own row may rise and fall: the search takes the FIRST adjacent pair that brackets the target, in either direction, never
    a position in the sorted values."""
    m = np.array([5.0, 9.0, 7.0, 3.0, 6.0, 12.0])
    fc = lambda t: hl1_areas._first_crossing("t", m, t)
    assert fc(8.0) == 0 and fc(9.0) == 0 and fc(7.5) == 0 and fc(4.0) == 2 and fc(3.0) == 2 and fc(10.0) == 4
    assert fc(6.5) == 0                                                               # not 3 or 4, where the sorted curve would put it
    for t in (2.9, 12.1):
        with pytest.raises(ValueError, match="no adjacent pair"):
            fc(t)
    x = np.arange(6.0) * 10.0
    v, t, slope = hl1_areas._interpolate_pair(x, m, 0, 8.0)                            # rising pair (5, 9) over (0, 10)
    assert (v, t, slope) == (7.5, 0.75, 0.4)
    v, t, slope = hl1_areas._interpolate_pair(x, m, 2, 4.0)                            # falling pair (7, 3) over (20, 30)
    assert (v, t, slope) == (27.5, 0.75, -0.4)
    assert hl1._pick_pair("t", m, 6.5) == 4                                           # hl1's rule for sorted curves lands on a later crossing


def test_arguments_are_checked_before_the_device():
    d = hl1_areas.demo_system(hours=24)
    L = hl1_areas.AreaSweepLevel
    ok = [L()]
    for kw in (dict(n_years=10, chains=3), dict(n_years=0), dict(n_years=10, start="cold"), dict(n_years=10, flow="dc"),
               dict(n_years=10, levels=[]), dict(n_years=10, levels=[L()] * 9), dict(n_years=10, levels=[L(load_shift=float("nan"))]),
               dict(n_years=10, levels=[L(load_scale=[1.0, float("inf")])]), dict(n_years=10, levels=[L(load_scale=[1.0, 1.0, 1.0])]),
               dict(n_years=10, levels=[L(load_shift=[[0.0, 0.0]])]), dict(n_years=10, levels=[L(tie_scale=-0.1)]),
               dict(n_years=10, levels=[L(tie_scale=float("nan"))]), dict(n_years=10, levels=[L(withheld=True)]),
               dict(n_years=10, withheld_units=[10]), dict(n_years=10, withheld_units=[-1]), dict(n_years=10, withheld_units=[3, 3]),
               dict(n_years=10, scaled_ties=[1]), dict(n_years=10, scaled_ties=[0, 0])):
        with pytest.raises(ValueError):
            hl1_areas.run_area_sweep(d, **{"levels": ok, **kw})
    with pytest.raises(ValueError):
        hl1_areas.level_system(d, L(withheld=True))
    alcc = lambda **kw: hl1_areas.area_load_carrying_capability(d, **{"area": 2, "target": 5.0, "n_years": 10, "bracket": (-50.0, 50.0), **kw})
    for kw in (dict(metric="lolf"), dict(row="tie"), dict(area=0), dict(area=3), dict(area="Area_Poor"), dict(bracket=(5.0, 5.0)),
               dict(bracket=(0.0, float("inf"))), dict(rounds=0), dict(chains=3), dict(start="cold")):
        with pytest.raises(ValueError):
            alcc(**kw)
    for kw in (dict(area=3), dict(metric="lolf"), dict(row="both"), dict(bracket=(3.0, 1.0)), dict(rounds=0), dict(chains=4)):
        with pytest.raises(ValueError):
            hl1_areas.interconnection_benefit(d, **{"area": 2, "n_years": 10, **kw})
    with pytest.raises(ValueError):                                                   # no tie at the area: the default bracket is empty
        hl1_areas.interconnection_benefit(hl1_areas.System(d.areas, []), 1, 10)
    for kw in (dict(units=[]), dict(units=[10]), dict(units=[2, 2]), dict(area=0), dict(metric="lolf"), dict(bracket=(3.0, 1.0)), dict(rounds=0)):
        with pytest.raises(ValueError):
            hl1_areas.unit_elcc(d, **{"units": [7], "area": 2, "n_years": 10, **kw})


def test_area_sweep_report():
    L = hl1_areas.AreaSweepLevel
    lv = [L(), L(load_shift=[0.0, -100.0], tie_scale=0.0, withheld=True)]
    yr = np.zeros((2, 4, 3, 3))
    sw = hl1_areas.AreaSweepResult(lv, (6,), (0,), "max_flow", 4, ["Area_Rich", "Area_Poor"],
                                   np.array([[66.0, 1095.13, 1098.9], [68.94, 3379.14, 3385.82]]),
                                   np.array([[14566.8, 161482.28, 176049.08], [14829.5, 622358.49, 637188.0]]),
                                   np.array([[1.5, 20.25, 21.0], [1.6, 40.0, 41.0]]), np.full((2, 3), 0.5), np.full((2, 3), 25.0),
                                   np.full((2, 3), 0.1), yr, 0.3)
    rows = hl1_areas.area_sweep_report(sw).splitlines()
    assert rows[1] == "=== MULTI-AREA SWEEP (INTERCONNECTED, max_flow) ==="
    assert rows[2].startswith("Level | Ties   | Fleet | Area       | LOLE (h/yr) +- SE")
    assert rows[4] == "0     | x1     | all   | Area_Rich  |      66.00 +- 0.50     |     14566.80 +- 25.00     |     1.5000"
    assert rows[6] == "0     | x1     | all   | SYSTEM     |    1098.90 +- 0.50     |    176049.08 +- 25.00     |    21.0000"
    assert rows[7] == "      load scale 1, shift 0 MW"
    assert rows[10].startswith("1     | x0     | w/o   | Area_Poor  |    3379.14")
    assert rows[12] == "      load scale 1, shift 0, -100 MW" and rows[-1] == "w/o: the fleet without units [6]"
