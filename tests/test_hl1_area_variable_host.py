"""Weather-year resources and storages in the areas of the HL1 multi-area chronology, without a GPU: the host model
(tests/tools/hl1_area_variable_model.py) against a pattern worked out by hand, against the models it is built on, and on the contract's
consequences C4 .. C6; the paths its fixtures reach; the exports and struct layouts (C compiler = ctypes = Julia); every ValueError of
hl1_area_variable.py before the engine is touched; the report."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

from powersystemsreliabilityassessment_amd import _abi, _lib, hl1, hl1_area_variable as AV, hl1_areas, hl1_storage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("hl1_area_variable_model", os.path.join(ROOT, "tests", "tools", "hl1_area_variable_model.py"))
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)
AM, TM, VM = M.AM, M.TM, M.VM
ISO, INTER, REF, MAXF = M.ISOLATED, M.INTERCONNECTED, M.REFERENCE, M.MAX_FLOW


def _model(s, out, wl, chains, policy, flow, storages=None, rs=None, lsh=None, start=M.STATIONARY, pick=M.PICK_RANDOM, counters=None, seed=8):
    return M.area_variable_model(seed, chains, s["units"], s["cap"], s["mttf"], s["mttr"], s["loads"], s["ties"], s["years"], start, policy, flow, out,
                                 s["resource_area"], wl, s["resource_scale"] if rs is None else rs, load_shift=lsh, pick=pick,
                                 storages=s["storages"] if storages is None else storages, tie_mttf=s["tie_mttf"], tie_mttr=s["tie_mttr"],
                                 counters=counters)[0]


def test_pattern_worked_out_by_hand():
    """Two areas, two weather years, two years of four hours, in dyadic numbers.  Area 0: units 8 + 8 MW against 10 MW; area 1: one 4 MW
    unit against (3, 5, 6, 7) MW, one resource, one storage (2 MW in and out, 4 MWh, lossless, 1 MWh at the start); a 1 MW tie.
    Year 0 draws weather year 1 (output 0, 2, 0, 0), year 1 weather year 0 (output 1, 1, 0, 0).  Unit 1 is DOWN on steps 3 .. 5, unit 2
    on step 8.
      step  m_0  m_1   after the tie   storage                      left (area 0, area 1)   state of charge
        1    6    1     6    1         charges 1                    -                        2
        2    6    1     6    1         charges 1                    -                        3
        3   -2   -2    -2   -2         delivers 2: served           2, 0                     1
        4   -2   -3    -2   -3         delivers 1                   2, 2                     0
        5   -2    2    -1    1         charges 1                    1, 0   (area 0's event runs over the year boundary)   1
        6    6    0     6    0         -                            -                        1
        7    6   -2     5   -1         delivers 1: served by import + storage   -            0
        8    6   -7     5   -6         empty                        0, 6                     0"""
    cap, lo = [8.0, 8.0, 4.0], [0, 2, 3]
    ud = np.zeros((3, 8), dtype=bool)
    ud[1, 2:5] = True
    ud[2, 7] = True
    out = np.array([[[1.0, 1.0, 0.0, 0.0]], [[0.0, 2.0, 0.0, 0.0]]])
    loads = np.array([[10.0] * 4, [3.0, 5.0, 6.0, 7.0]])
    m = M.step_margins(ud, lo, cap, [1, 0], loads, out, [1], None, [1.0], [1.0, 1.0], [0.0, 0.0])
    assert m.tolist() == [[6, 1], [6, 1], [-2, -2], [-2, -3], [-2, 2], [6, 0], [6, -2], [6, -7]]
    st = [(1, (2.0, 2.0, 4.0, 1.0, 1.0, 1.0))]
    trace, cnt = [], M.new_counters(2)
    rec = M.area_variable_chain(m, None, 2, [(0, 1, 1.0)], 4, 2, INTER, MAXF, st, cnt, trace)
    assert [t[0][0] for t in trace] == [2, 3, 1, 0, 1, 1, 0, 0]
    assert [t[1] for t in trace] == [(0, 0), (0, 0), (2, 0), (2, 2), (1, 0), (0, 0), (0, 0), (0, 6)]
    #                       lole eue lolf served out in
    assert rec[0].tolist() == [[2, 4, 1, 0, 0, 0], [1, 2, 1, 1, 3, 2], [2, 6, 1, 0, 3, 2]]
    assert rec[1].tolist() == [[1, 1, 0, 0, 0, 0], [1, 6, 1, 1, 1, 1], [2, 7, 1, 1, 1, 1]]
    assert cnt["transfer_steps"] == 3 and cnt["import_then_storage"] == 1 and cnt["act_steps"] == 6
    assert cnt["served"] == [0, 2, 1] and cnt["left"] == [3, 2, 4] and cnt["short"] == [3, 4, 5]
    # the same margins under REFERENCE flow and ISOLATED
    assert np.array_equal(M.area_variable_chain(m, None, 2, [(0, 1, 1.0)], 4, 2, INTER, REF, st), rec)
    iso = M.area_variable_chain(m, None, 2, [(0, 1, 1.0)], 4, 2, ISO, REF, st)
    #   step 5: no export, area 0 is 2 short and area 1 charges 2 (2 MWh); step 7: delivers 2, served; step 8: empty, 7 left
    assert iso[1].tolist() == [[1, 2, 0, 0, 0, 0], [1, 7, 1, 1, 2, 2], [2, 9, 1, 1, 2, 2]] and np.array_equal(iso[0], rec[0])
    # the tie DOWN on step 7 only: nothing is imported there, the storage delivers its 1 MWh, 1 MW is left
    td = np.zeros((1, 8), dtype=bool)
    td[0, 6] = True
    down = M.area_variable_chain(m, td, 2, [(0, 1, 1.0)], 4, 2, INTER, MAXF, st)
    assert down[1].tolist() == [[1, 1, 0, 0, 0, 0], [2, 7, 1, 0, 1, 1], [3, 8, 1, 0, 1, 1]]


def test_solve_step_agrees_with_solve_batch():
    """The one-step transfer solve of the model against hl1_area_model.solve_batch on random margins of 2 .. 5 areas, both flows."""
    rng = np.random.default_rng(4)
    for n in (2, 3, 5):
        ties = [(i, j, float(rng.integers(0, 4)) * 2.5) for i in range(n) for j in range(i + 1, n) if rng.uniform() < 0.8]
        T = AM.topology(n, ties)
        m = np.round(rng.normal(0.0, 6.0, (300, n)) * 4.0) / 4.0
        for flow in (REF, MAXF):
            want = AM.solve_batch(m, T, INTER, flow)
            got = np.array([M.solve_step(row, T, flow) for row in m])
            assert np.array_equal(np.where(got < 0, -got, 0.0), want)
            assert np.allclose(got.sum(1), m.sum(1))               # transfers move margin, they make none


def test_model_reduces_to_the_models_it_is_built_on():
    """No resource and no storage: hl1_tie_model.interval_model (C1 on the host).  One area: hl1_variable_model.variable_model (C2)."""
    s = M.shape("a3")
    z = np.zeros((1, 0, s["loads"].shape[1]))
    for policy, flow in ((ISO, REF), (INTER, REF), (INTER, MAXF)):
        rec = M.area_variable_model(3, range(5, 8), s["units"], s["cap"], s["mttf"], s["mttr"], s["loads"], s["ties"], 3, M.ALL_UP, policy, flow, z, [],
                                    tie_mttf=s["tie_mttf"], tie_mttr=s["tie_mttr"])[0]
        ref = TM.interval_model(3, range(5, 8), s["units"], s["cap"], s["mttf"], s["mttr"], s["loads"], s["ties"], s["tie_mttf"], s["tie_mttr"], 3,
                                M.ALL_UP, policy, flow)
        assert np.array_equal(rec[..., :3], ref) and not rec[..., 3:].any()
    cap, mttf, mttr, load = AM.SEQ.small_fleet()
    st = [(20.0, 20.0, 60.0, 0.9, 0.95, 60.0), (10.0, 15.0, 30.0, 0.85, 1.0, 0.0)]
    for pick in (M.PICK_RANDOM, M.PICK_CYCLE):
        out, wl = M.library(load[None, :], 3, [0, 0], 21, True)
        one, w1 = VM.variable_model(4, range(2, 6), cap, mttf, mttr, load, 3, M.STATIONARY, out, wl[:, 0, :], [1.0, 0.5], pick, st, 1.0625, -3.5)
        rec, w = M.area_variable_model(4, range(2, 6), [6], cap, mttf, mttr, load[None, :], [], 3, M.STATIONARY, INTER, REF, out, [0, 0], wl, [1.0, 0.5],
                                       [1.0625], [-3.5], pick, [(0, x) for x in st])
        assert np.array_equal(rec[:, 0], one) and np.array_equal(rec[:, 1], one) and np.array_equal(w, w1) and one[:, 3].sum() > 0


@pytest.mark.parametrize("name", ["a2", "a3", "a5"])
def test_c4_c5_on_the_model(name):
    s = M.shape(name)
    n = len(s["units"])
    out, wl = M.library(s["loads"], s["n_weather"], s["resource_area"], 11, True)
    for policy, flow in ((ISO, REF), (INTER, MAXF), (INTER, REF)):
        rec = _model(s, out, wl, range(3, 6), policy, flow)
        rec0 = _model(s, out, wl, range(3, 6), policy, flow, storages=[])
        assert np.array_equal(rec[..., 3] + rec[..., 0], rec0[..., 0]) and not rec0[..., 3:].any() and rec[..., 3].sum() > 0
        unable = [(a % n, st) for a, st in enumerate([(5.0, 0.0, 10.0, 0.9, 0.9, 10.0), (2.0, 3.0, 0.0, 0.7, 0.7, 0.0), (0.0, 4.0, 9.0, 1.0, 1.0, 0.0)])]
        assert np.array_equal(_model(s, out, wl, range(3, 6), policy, flow, storages=unable), rec0)
        # no discharge but room left: by the step rule it charges, and never delivers
        rec5 = _model(s, out, wl, range(3, 6), policy, flow, storages=[(n - 1, (5.0, 0.0, 10.0, 0.9, 0.9, 5.0))])
        assert np.array_equal(rec5[..., :5], rec0[..., :5]) and rec5[:, n - 1, 5].sum() > 0


def test_c6_on_the_model():
    s = M.shape("a2")
    s["cap"] = np.array([60.0, 50.0, 40.0, 40.0, 25.0, 15.0])
    s["loads"] = np.round(s["loads"] * 8.0) / 8.0
    H = s["loads"].shape[1]
    other = np.round(np.random.default_rng(2).uniform(0.0, 6.0, (3, 1, H)) * 16.0) / 16.0
    st = [(1, (8.0, 8.0, 16.0, 1.0, 1.0, 8.0))]
    for a, p in ((0, 12.5), (1, 6.75)):
        s["resource_area"] = [1 - a, a]
        out = np.concatenate([other, np.full((3, 1, H), p)], axis=1)
        sh = [0.5, -1.25]
        with_p = _model(s, out, None, range(8), INTER, MAXF, storages=st, rs=[1.0, 1.0], lsh=sh)
        sh[a] -= p
        shifted = _model(s, out, None, range(8), INTER, MAXF, storages=st, rs=[1.0, 0.0], lsh=sh)
        assert np.array_equal(with_p, shifted) and with_p[:, 2, 0].sum() > 0


def test_the_fixtures_reach_every_counter():
    """Over the four shapes of the device tests: quiet and serial groups, steps the serial stage visits, transfers, an import followed by
    a discharge, every able storage discharging and charging, served and left hours in some area and for the system."""
    tot = {}
    for name, nch in (("a2", 5), ("a3", 4), ("a5", 3), ("rts96", 2)):
        s = M.shape(name)
        out, wl = M.library(s["loads"], s["n_weather"], s["resource_area"], 11, False)
        cnt = M.new_counters(len(s["units"]))
        _model(s, out, wl, range(1000, 1000 + nch), INTER, MAXF, counters=cnt)
        _model(s, out, wl, range(1000, 1000 + nch), ISO, REF, counters=cnt)        # the device tests run both policies on every shape
        for k in ("groups", "quiet_groups", "serial_groups", "act_steps", "transfer_steps", "import_then_storage"):
            assert name == "rts96" or k == "quiet_groups" or cnt[k] > 0, (name, k)
            tot[k] = tot.get(k, 0) + cnt[k]
        assert cnt["groups"] == cnt["quiet_groups"] + cnt["serial_groups"]
        assert cnt["served"][-1] > 0 and cnt["left"][-1] > 0 and max(cnt["served"][:-1]) > 0 and all(x + y == z for x, y, z in zip(cnt["served"], cnt["left"], cnt["short"]))
        able = [i for i, (_, q) in enumerate(s["storages"]) if q[1] > 0 and q[2] > 0]
        assert all(cnt["discharge"][i] > 0 for i in able), (name, cnt["discharge"])
        assert all(cnt["charge"][i] > 0 for i, (_, q) in enumerate(s["storages"]) if q[0] > 0 and q[2] > 0 and i in able), (name, cnt["charge"])
    assert all(v > 0 for v in tot.values()), tot


def test_expectation_power():
    """How many one-year chains tests/test_hl1_area_variable.py::test_exact_expectation needs so that the no-resource expectation lies
    more than 4.5 SE from the expectation with the resources: from the per-year spread of 300 model chains, with a factor 4 in hand."""
    spec = importlib.util.spec_from_file_location("gpu_tests", os.path.join(ROOT, "tests", "test_hl1_area_variable.py"))
    T = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(T)
    case = T._expect_case()
    units, cap, mttf, mttr, loads, ties, out, wl = case
    exact, without = T._expectations(case)
    rec = M.area_variable_model(5, range(300), units, cap, mttf, mttr, loads, ties, 1, M.STATIONARY, INTER, MAXF, out, [0, 1], wl, [1.0, 1.0],
                                pick=M.PICK_CYCLE)[0]
    need = (4.5 * rec[:, :, :2].std(0, ddof=1) / np.abs(without - exact)) ** 2
    assert need.max() * 4.0 < T.EXPECT_CHAINS and T.EXPECT_CHAINS % 3 == 0, need


# ---- ABI --------------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "relmc.h")).read()
    jl = open(os.path.join(ROOT, "julia", "RelMC.jl")).read()
    for sym in ("relmc_hl1_area_var_load", "relmc_hl1_area_var"):
        assert re.search(r"\b%s\s*\(" % sym, hdr) and sym in _lib.EXPORTS and (":" + sym + ",") in jl, sym
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = _lib.load()
    assert all(hasattr(L, s) for s in ("relmc_hl1_area_var_load", "relmc_hl1_area_var"))
    assert len(L.relmc_hl1_area_var_load.argtypes) == 8 and len(L.relmc_hl1_area_var.argtypes) == 13


@pytest.mark.parametrize("cname,mirror,jname,size", [("relmc_hl1_area_var_opts", _abi.Hl1AreaVarOpts, "Hl1AreaVarOpts", 208),
                                                     ("relmc_hl1_area_storage", _abi.Hl1AreaStorage, "Hl1AreaStorage", 56)])
def test_struct_layout_matches_the_mirrors(tmp_path, cname, mirror, jname, size):
    """sizeof / offsetof from the C compiler == the ctypes mirror (field names and order included) == julia/RelMC.jl's struct and table."""
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "relmc.h"', 'int main(void) {', f'printf("%zu", sizeof({cname}));']
    prog += [f'printf(" %zu", offsetof({cname}, {f}));' for f, _ in mirror._fields_]
    prog.append('printf("\\n"); return 0; }')
    src = tmp_path / "layout.c"
    src.write_text("\n".join(prog))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    assert got == [C.sizeof(mirror)] + [getattr(mirror, f).offset for f, _ in mirror._fields_] and got[0] == size
    jl = open(os.path.join(ROOT, "julia", "RelMC.jl")).read()
    body = re.search(r"struct %s\n(.*?)\nend" % jname, jl, re.S).group(1)
    jtypes = {C.c_double: "Cdouble", C.c_int32: "Int32", C.c_double * 8: "NTuple{8,Cdouble}", _abi.Hl1Storage: "Hl1Storage"}
    assert re.findall(r"(\w+)::([\w{},]+)", body) == [(f, jtypes[t]) for f, t in mirror._fields_]
    row = re.search(r'\("%s", (\d+), \[(.*?)\]\),' % cname, jl).groups()
    assert [int(row[0])] + [int(x) for x in re.findall(r'\("\w+", (\d+)\)', row[1])] == got
    assert re.findall(r'\("(\w+)", \d+\)', row[1]) == [f for f, _ in mirror._fields_]


# ---- the Python layer: every ValueError before the engine is touched -----------------------------------------------------------------
class _Untouchable:
    """Stands in for the engine: any use of it fails the test."""
    def __getattr__(self, name):
        raise AssertionError(f"the engine was touched ({name}) before the arguments were checked")


def _small_system(hours=48):
    h = np.arange(hours)
    a = hl1_areas.Area(1, "West", [hl1.Generator(i, 50.0, 400.0, 40.0) for i in range(1, 4)], 100.0 + 20.0 * np.sin(2 * np.pi * h / 24.0))
    b = hl1_areas.Area(2, "East", [hl1.Generator(i, 30.0, 300.0, 30.0) for i in range(1, 4)], 60.0 + 15.0 * np.sin(2 * np.pi * h / 24.0))
    return hl1_areas.System([a, b], [hl1_areas.TieLine(1, 2, 20.0)])


def test_every_value_error():
    sysm = _small_system()
    out = np.ones((2, 2, 48))
    w = AV.AreaWeatherYears(out, (1, 2))
    battery = hl1_storage.Storage(10.0, 10.0, 40.0, 0.9, 0.9)
    eng = _Untouchable()
    run = lambda **kw: AV.run_area_variable(kw.pop("sys", sysm), kw.pop("policy", hl1_areas.INTERCONNECTED), kw.pop("weather", w), kw.pop("n_years", 4),
                                            engine=eng, **kw)
    with pytest.raises(ValueError, match="3-dimensional|not 2-dimensional"):
        AV.AreaWeatherYears(np.ones((2, 48)), (1,))
    with pytest.raises(ValueError, match="resource areas"):
        AV.AreaWeatherYears(out, (1,))
    bad_out = out.copy(); bad_out[1, 0, 7] = -1.0
    nan_out = out.copy(); nan_out[0, 1, 3] = np.nan
    bad_load = np.ones((2, 2, 48)); bad_load[1, 1, 9] = np.inf
    cases = [
        (dict(n_years=0), "positive multiple"), (dict(n_years=5, chains=2), "positive multiple"), (dict(start="warm"), "start"),
        (dict(flow="dc"), "flow"), (dict(policy=2), "policy"), (dict(pick="first"), "pick"),
        (dict(weather=AV.AreaWeatherYears(np.ones((257, 1, 48)), (1,))), "n_weather 257"),
        (dict(weather=AV.AreaWeatherYears(np.ones((1, 9, 48)), (1,) * 9)), "n_resources 9"),
        (dict(weather=AV.AreaWeatherYears(out, (1, 3))), "resource 1 is in area 3"), (dict(weather=AV.AreaWeatherYears(out, (0, 1))), "resource 0 is in area 0"),
        (dict(weather=AV.AreaWeatherYears(bad_out, (1, 2))), "weather year 1, resource 0, hour 7 is negative"),
        (dict(weather=AV.AreaWeatherYears(nan_out, (1, 2))), "weather year 0, resource 1, hour 3 is not finite"),
        (dict(weather=AV.AreaWeatherYears(out, (1, 2), np.ones((2, 48)))), "load_mw must be"),
        (dict(weather=AV.AreaWeatherYears(out, (1, 2), bad_load)), "weather year 1, area 2, hour 9 not finite"),
        (dict(weather=AV.AreaWeatherYears(np.ones((2, 2, 24)), (1, 2))), "48 hours, the weather years 24"),
        (dict(resource_scale=[1.0]), "1 resource scales"), (dict(resource_scale=[1.0, -1.0]), "resource_scale 1 is negative"),
        (dict(resource_scale=[np.inf, 1.0]), "resource_scale 0 not finite"),
        (dict(load_scale=[1.0]), "load_scale for 2 areas"), (dict(load_scale=[1.0, np.nan]), "load_scale of area 2 not finite"),
        (dict(load_shift=[np.inf, 0.0]), "load_shift of area 1 not finite"),
        (dict(storages=[AV.AreaStorage(1, battery)] * 9), "9 storages"), (dict(storages=[AV.AreaStorage(3, battery)]), "storage 0 is in area 3"),
        (dict(storages=[AV.AreaStorage(0, battery)]), "storage 0 is in area 0"),
        (dict(storages=[AV.AreaStorage(1, battery), AV.AreaStorage(2, hl1_storage.Storage(1.0, 1.0, 4.0, 1.5, 1.0))]), "eta_charge of storage 1"),
        (dict(storages=[AV.AreaStorage(2, hl1_storage.Storage(1.0, -1.0, 4.0))]), "discharge_mw of storage 0 is negative"),
        (dict(storages=[AV.AreaStorage(2, hl1_storage.Storage(1.0, 1.0, 4.0, 1.0, 1.0, 5.0))]), "soc0_mwh of storage 0"),
    ]
    for kw, word in cases:
        with pytest.raises(ValueError, match=re.escape(word)):
            run(**kw)
    elcc = lambda **kw: AV.area_resource_elcc(sysm, kw.pop("weather", w), kw.pop("area", 2), kw.pop("n_years", 4), engine=eng, **kw)
    for kw, word in [(dict(resources=[0], metric="lolf"), "metric"), (dict(resources=[0], row="tie"), "row"), (dict(resources=[0], area=3), "area must be"),
                     (dict(resources=[0], area=0), "area must be"), (dict(resources=[2]), "resources must be indices"), (dict(), "no resource and no storage"),
                     (dict(resources=[0], n_years=0), "positive multiple"), (dict(resources=[0], bracket=(3.0, 1.0)), "bracket"),
                     (dict(resources=[0], rounds=0), "rounds"), (dict(resources=[0], resource_scale=[0.0, 1.0]), "can deliver nothing"),
                     (dict(storages=[AV.AreaStorage(5, battery)]), "storage 0 is in area 5"),
                     (dict(resources=[0], weather=AV.AreaWeatherYears(np.ones((2, 2, 24)), (1, 2))), "weather years 24")]:
        with pytest.raises(ValueError, match=re.escape(word)):
            elcc(**kw)
    with pytest.raises(ValueError, match="n_weather"):
        AV.synthetic_area_weather(sysm, 0)
    five = hl1_areas.System([hl1_areas.Area(k + 1, str(k), sysm.areas[0].generators, sysm.areas[0].hourly_load) for k in range(5)], [])
    with pytest.raises(ValueError, match="10 resources"):
        AV.synthetic_area_weather(five, 2)


def test_synthetic_library_and_report():
    sysm = _small_system()
    lib = AV.synthetic_area_weather(sysm, 3, solar_mw=20.0, wind_mw=10.0, load_curves=True)
    assert lib.output_mw.shape == (3, 4, 48) and lib.resource_area == (1, 1, 2, 2) and lib.load_mw.shape == (3, 2, 48)
    assert lib.names == ("solar_West", "wind_West", "solar_East", "wind_East") and lib.output_mw.min() >= 0.0 and lib.output_mw[:, 0].max() <= 20.0
    assert not np.array_equal(lib.output_mw[:, 1], lib.output_mw[:, 3])                 # every area from its own seed
    assert AV._area_weather("t", lib, 2, 48) is lib
    res = [hl1_areas.AreaResult("West", 2.0, 30.0), hl1_areas.AreaResult("East", 5.0, 80.0)]
    base = hl1_areas.MultiAreaResult(hl1_areas.INTERCONNECTED, "max_flow", res, np.zeros(2), np.zeros(2), 6.0, 110.0, 1.0, 6.0, 0.0)
    res1 = [hl1_areas.AreaResult("West", 1.5, 20.0), hl1_areas.AreaResult("East", 2.25, 31.5)]
    r = AV.AreaVariableResult(hl1_areas.INTERCONNECTED, "max_flow", res1, np.zeros(2), np.zeros(2), 3.5, 51.5, 1.0, 3.5, 0.0,
                              served_hours=np.array([0.0, 1.75, 1.25]), discharged_mwh=np.array([0.0, 41.0, 41.0]), charged_mwh=np.array([0.0, 52.5, 52.5]),
                              year_weather=np.array([0, 2, 2, 1], dtype=np.int32), resource_scale=(1.0, 0.0, 1.0, 1.0),
                              storages=(AV.AreaStorage(2, hl1_storage.Storage(10.0, 10.0, 40.0)),), pick="cycle")
    txt = AV.area_variable_report(base, r)
    lines = txt.splitlines()
    east = next(ln for ln in lines if ln.startswith("East"))
    assert "5.0000" in east and "2.2500" in east and "80.00" in east and "31.50" in east and "1.7500" in east and "41.00 / 52.50" in east
    system = next(ln for ln in lines if ln.startswith("System"))
    assert "6.0000" in system and "3.5000" in system and "110.00" in system and "51.50" in system
    assert "INTERCONNECTED, max_flow" in txt and "3 resources, 1 storage, 3 weather years drawn (cycle)" in txt and "after the ties" in txt
