"""Three-state units on the HL1 sequential chronology (relmc_hl1_ms_load / relmc_hl1_ms_seq) without a GPU: the host model's interval form
against its hour loop and against the two-state model, the stationary law, the three-term COPT, the exact loss frequency of a small
fleet, the C ABI's exports and struct layouts, and the Python argument checks that need no device."""
import ctypes as C
import importlib.util
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

from powersystemsreliabilityassessment_amd import _abi, _lib, hl1, hl1_multistate as ms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("hl1_multistate_model", os.path.join(ROOT, "tests", "tools", "hl1_multistate_model.py"))
MM = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(MM)
SEQ = MM.SEQ


def _tuples(units):
    return [(u.capacity, u.derated_capacity, u.mean_h, u.first_p) for u in units]


def _objects(units):
    return [ms.MultiStateUnit.from_means(k, *u) for k, u in enumerate(units)]


@pytest.mark.parametrize("start", [MM.ALL_UP, MM.STATIONARY])
@pytest.mark.parametrize("fleet,chains,years", [("six", [0, 1, 2, 3, 1 << 33], 4), ("rts24", [0, 7], 2), ("short", [0, 5], 3)])
def test_interval_form_equals_the_hour_loop(fleet, chains, years, start):
    """(a) == (b): every per-year loss-hour, loss-event, derated and down unit-hour count, EUE to 1e-12, the state carried across years."""
    units, load = (MM.six_unit_fleet() if fleet == "six" else MM.short_fleet() if fleet == "short"
                   else (_tuples(ms.derated_rts24()), hl1.rts24_load().hourly_load))
    a = MM.interval_model(5, chains, units, load, years, start)
    b = np.concatenate([MM.literal_chain(5, c, units, load, years, start) for c in chains])
    np.testing.assert_array_equal(a[:, [0, 2, 3, 4]], b[:, [0, 2, 3, 4]])
    np.testing.assert_allclose(a[:, 1], b[:, 1], rtol=1e-12, atol=1e-9)
    assert a[:, 3].sum() > 0 and a[:, 4].sum() > 0                                 # the chains do see derated and down hours
    assert fleet == "rts24" or (a[:, 0].sum() > 0 and a[:, 2].sum() > 0)           # (four chain years of RTS-24 may see no loss)


@pytest.mark.parametrize("start", [MM.ALL_UP, MM.STATIONARY])
@pytest.mark.parametrize("fleet", ["small", "rts24"])
def test_two_state_units_give_the_sequential_model_exactly(fleet, start):
    if fleet == "small":
        cap, mttf, mttr, load = SEQ.small_fleet()
    else:
        gens = hl1.rts24_generators()
        cap, mttf, mttr = (np.array([getattr(g, f) for g in gens]) for f in ("capacity", "mttf", "mttr"))
        load = hl1.rts24_load().hourly_load
    units = [MM.two_state(c, f, r) for c, f, r in zip(cap, mttf, mttr)]
    chains, years = ([0, 3, 1 << 40], 3) if fleet == "small" else ([2], 2)
    a = MM.interval_model(9, chains, units, load, years, start)
    L, E, F = SEQ.interval_model(9, chains, cap, mttf, mttr, load, years, start)
    assert a[:, 0].tobytes() == L.tobytes() and a[:, 1].tobytes() == E.tobytes() and a[:, 2].tobytes() == F.tobytes()
    assert not a[:, 3].any() and a[:, 4].sum() > 0
    for u, f, r in zip(units, mttf, mttr):                                          # pi_2 by hl1_units_fill's very expression
        assert MM.thresholds(u) == (r / (f + r), r / (f + r), 0.0)


def test_stationary_law_is_the_null_space_of_the_generator():
    fleets = MM.six_unit_fleet()[0] + MM.short_fleet()[0] + MM.lolf_fleet()[0] + _tuples(ms.derated_rts24())
    seen = set()
    for u in fleets:
        obj = ms.MultiStateUnit.from_means("u", *u)
        pi = ms.stationary(obj)
        assert pi.sum() == pytest.approx(1.0, abs=1e-15) and (pi >= 0).all()
        p2, p12, p1 = MM.thresholds(u)
        assert (pi[2], pi[1]) == (p2, p1) and p12 == p2 + p1                        # the package and the model agree to the bit
        reach = {0} | ({1} if pi[1] > 0 else set()) | ({2} if pi[2] > 0 else set())
        seen.add(tuple(sorted(reach)))
        idx = sorted(reach)
        Q = MM.generator_matrix(u)[np.ix_(idx, idx)]
        assert np.abs(Q.sum(1)).max() < 1e-15 * np.abs(Q).max()                     # nothing leaves the reachable states
        assert np.abs(pi[idx] @ Q).max() < 1e-15 * np.abs(Q).max()
        # the rate matrix round-trips through the constructor
        back = ms.MultiStateUnit("u", obj.capacity, obj.derated_capacity, obj.rates)
        for s in idx:
            assert back.mean_h[s] == pytest.approx(obj.mean_h[s], rel=1e-14) and back.first_p[s] == pytest.approx(obj.first_p[s], abs=1e-15)
    assert seen == {(0, 1), (0, 2), (0, 1, 2)}
    g = hl1.Generator(7, 50.0, 1960.0, 40.0)
    u = ms.MultiStateUnit.from_generator(g)
    assert (u.mean_h[0], u.mean_h[2], u.first_p) == (1960.0, 40.0, (1.0, 1.0, 1.0)) and ms.stationary(u)[2] == 40.0 / (1960.0 + 40.0)


def test_analytical_multistate():
    """Two-state RTS-24: hl1.run_analytical's numbers (its for_rate is lam / (lam + mu) with lam = 1 / mttf, mu = 1 / mttr, the law here
    mttr / (mttf + mttr): the same number up to two roundings per unit, so the indices agree to 1e-12).  Two units, one derated:
    the 9 joint states by hand."""
    gens, load = hl1.rts24_generators(), hl1.rts24_load()
    for step in (10.0, 1.0):
        a = ms.run_analytical_multistate([ms.MultiStateUnit.from_generator(g) for g in gens], load, step)
        b = hl1.run_analytical(gens, load, step)
        assert a.lole_hours_yr == pytest.approx(b.lole_hours_yr, rel=1e-12) and a.eue_mwh_yr == pytest.approx(b.eue_mwh_yr, rel=1e-12)
    full = ms.run_analytical_multistate(ms.derated_rts24(), load, 1.0)
    ref = hl1.run_analytical(gens, load, 1.0)
    assert 0 < full.lole_hours_yr and full.lole_hours_yr != pytest.approx(ref.lole_hours_yr, rel=1e-3)
    units = _objects([MM.three_state(40.0, 25.0, 300.0, 30.0), MM.three_state(30.0, 10.0, 200.0, 50.0, scale=(0.5, 1.0, 1.0, 1.0, 2.0, 0.5))])
    curve = np.array([20.0, 34.5, 35.0, 41.0, 55.0, 69.5, 70.0, 75.0])
    pis = [ms.stationary(u) for u in units]
    lole = eue = 0.0
    for s0, s1 in itertools.product(range(3), repeat=2):                            # the 9 joint states
        avail = (units[0].capacity, units[0].derated_capacity, 0.0)[s0] + (units[1].capacity, units[1].derated_capacity, 0.0)[s1]
        p = pis[0][s0] * pis[1][s1]
        lole += p * (avail < curve).sum()
        eue += p * np.maximum(curve - avail, 0.0).sum()
    got = ms.run_analytical_multistate(units, hl1.LoadModel(curve), step_size=0.5)   # every capacity and load on the 0.5 MW grid
    assert got.lole_hours_yr == pytest.approx(lole, rel=1e-12) and got.eue_mwh_yr == pytest.approx(eue, rel=1e-12)


def test_model_matches_the_exact_small_fleet_expectations():
    """(a) against (c): stationary LOLE, EUE and loss events per year of four three-state units within 4.5 standard errors (4000 one-year
    chains); the one-hour transition matrices are proper, and the enumeration's LOLE / EUE are the COPT's."""
    units, load = MM.lolf_fleet()
    for u in units:
        P = MM.expm(MM.generator_matrix(u))
        p2, _, p1 = MM.thresholds(u)
        pi = np.array([1.0 - p1 - p2, p1, p2])
        assert np.abs(P.sum(1) - 1.0).max() < 1e-14 and (P > 0).all() and np.abs(pi @ P - pi).max() < 1e-15
        Q = MM.generator_matrix(u)
        assert np.abs(MM.expm(2.0 * Q) - P @ P).max() < 1e-14
    rec = MM.interval_model(2, range(4000), units, load, 1, MM.STATIONARY)
    el, ee, ef = MM.small_fleet_stationary(units, load)
    for q, e in ((0, el), (1, ee), (2, ef)):
        x = rec[:, q]
        assert abs(x.mean() - e) < 4.5 * x.std(ddof=1) / np.sqrt(x.size), (q, x.mean(), e)
    pi1 = sum(MM.thresholds(u)[2] for u in units)
    pi2 = sum(MM.thresholds(u)[0] for u in units)
    for q, e in ((3, len(load) * pi1), (4, len(load) * pi2)):
        x = rec[:, q]
        assert abs(x.mean() - e) < 4.5 * x.std(ddof=1) / np.sqrt(x.size), (q, x.mean(), e)
    copt = ms.run_analytical_multistate(_objects(units), hl1.LoadModel(load), step_size=0.5)
    assert (el, ee) == pytest.approx((copt.lole_hours_yr, copt.eue_mwh_yr), rel=1e-10)


def test_short_fixture_reaches_every_edge_case():
    units, load = MM.short_fleet()
    for start in (MM.ALL_UP, MM.STATIONARY):
        reached = MM.path_counts(7, range(8), units, load, 3, start)
        assert all(v > 0 for v in reached.values()), reached


def test_library_exports_the_multistate_entry_points():
    hdr = open(os.path.join(ROOT, "include", "relmc.h")).read()
    jl = open(os.path.join(ROOT, "julia", "RelMC.jl")).read()
    for s in ("relmc_hl1_ms_load", "relmc_hl1_ms_seq"):
        assert re.search(r"\b" + s + r"\s*\(", hdr), s
        assert s in _lib.EXPORTS and ":" + s in jl
    assert "#define RELMC_HL1_MS_MAX_HOURS 1073741824" in hdr and _abi.HL1_MS_MAX_HOURS == 1073741824
    assert "#define RELMC_HL1_MS_BRANCH_TAG 0x50000000u" in hdr and _abi.HL1_MS_BRANCH_TAG == 0x50000000 == MM.BRANCH_TAG
    csrc = os.path.join(ROOT, "powersystemsreliabilityassessment_amd", "csrc")
    tags = set()
    for name in os.listdir(csrc):                                                   # no other kernel's Philox tag is the branch stream's
        if name.endswith((".h", ".hip")):
            tags |= set(re.findall(r"\|\s*(0x[0-9a-fA-F]{8})u", open(os.path.join(csrc, name)).read()))
    assert "0x50000000" not in {t.lower() for t in tags} and {"0x80000000", "0x40000000"} <= {t.lower() for t in tags}
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = _lib.load()
    assert hasattr(L, "relmc_hl1_ms_load") and hasattr(L, "relmc_hl1_ms_seq")


def test_multistate_struct_layouts_match_the_mirrors(tmp_path):
    """sizeof / offsetof of the three structs from the C compiler == the ctypes mirrors (field names and order included) == the field
    lists of julia/RelMC.jl's structs."""
    pairs = [("relmc_hl1_ms_unit", _abi.Hl1MsUnit, "Hl1MsUnit"), ("relmc_hl1_ms_year", _abi.Hl1MsYear, "Hl1MsYear"),
             ("relmc_hl1_ms_acc", _abi.Hl1MsAcc, "Hl1MsAcc")]
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
    jtypes = {C.c_double: "Cdouble", C.c_int64: "Int64", C.c_double * 3: "NTuple{3,Cdouble}"}
    for (name, m, jname), line in zip(pairs, lines):
        got = [int(x) for x in line.split()]
        assert got == [C.sizeof(m)] + [getattr(m, f).offset for f, _ in m._fields_], name
        body = re.search(r"struct %s\n(.*?)\n(?:    \w+\(\) = new\(\)\n)?end" % jname, jl, re.S).group(1)
        assert re.findall(r"(\w+)::([\w{},]+)", body) == [(f, jtypes[t]) for f, t in m._fields_], name
    assert [int(ln.split()[0]) for ln in lines] == [64, 16, 88]


class _Untouchable:
    """Stands in for the engine: any use of it fails the test."""
    def __getattr__(self, name):
        raise AssertionError(f"the engine was touched ({name}) before the arguments were checked")


def test_arguments_are_checked_before_the_engine():
    load = hl1.rts24_load()
    ok = ms.derated_rts24()
    U = ms.MultiStateUnit.from_means
    three = ((300.0, 30.0, 60.0), (0.5, 0.5, 0.5))
    nan, inf = float("nan"), float("inf")
    bad_units = [
        [U(0, nan, 0.0, *three)], [U(0, 100.0, inf, *three)], [U(0, 100.0, 50.0, (300.0, nan, 60.0), three[1])],
        [U(0, 100.0, 50.0, three[0], (0.5, 0.5, -inf))],
        [U(0, 100.0, -1.0, *three)], [U(0, 100.0, 100.5, *three)],                           # derated outside [0, capacity]
        [U(0, 100.0, 50.0, three[0], (1.5, 0.5, 0.5))], [U(0, 100.0, 50.0, three[0], (0.5, -0.1, 0.5))],
        [U(0, 100.0, 50.0, three[0], (0.5, 0.5, 1.0 + 2.0 ** -52))],
        [U(0, 100.0, 50.0, (0.0, 30.0, 60.0), three[1])], [U(0, 100.0, 50.0, (300.0, -2.0, 60.0), three[1])],
        [U(0, 100.0, 50.0, (300.0, 30.0, 0.0), three[1])],
        [U(0, 100.0, 50.0, three[0], (0.5, 0.0, 0.0))],                                      # DERATED <-> DOWN for ever
        ok + [U(0, 100.0, 50.0, (300.0, nan, 60.0), (1.0, 1.0, 1.0))],                       # an unreachable state's field must still be finite
        ok * 4 + ok[:1],                                                                     # 129 units
        [], [hl1.Generator(1, 50.0, 100.0, 10.0)],
    ]
    for units in bad_units:
        with pytest.raises(ValueError):
            ms.run_sequential_multistate(units, load, 10, engine=_Untouchable())
    for kw in (dict(years=10, chains=3), dict(years=0), dict(years=10, start="cold")):
        with pytest.raises(ValueError):
            ms.run_sequential_multistate(ok, load, **{"engine": _Untouchable(), **kw})
    with pytest.raises(ValueError, match="hour 3"):
        ms.run_sequential_multistate(ok, hl1.LoadModel(np.array([1.0, 2.0, 3.0, nan])), 10, engine=_Untouchable())
    with pytest.raises(ValueError, match="first_p of state DOWN of unit 32"):
        ms.run_sequential_multistate(ok + [U(0, 100.0, 50.0, three[0], (0.5, 0.5, 2.0))], load, 10, engine=_Untouchable())
    with pytest.raises(ValueError, match="cannot return to UP"):
        ms.run_analytical_multistate([U(0, 100.0, 50.0, three[0], (0.5, 0.0, 0.0))], load)
    with pytest.raises(ValueError):
        ms.run_analytical_multistate(ok, load, step_size=0.0)
    # what is ignored: the fields of a state that cannot be reached from UP
    assert ms.stationary(U(0, 100.0, 0.0, (300.0, -4.0, 60.0), (1.0, 9.0, 1.0)))[1] == 0.0
    assert ms.stationary(U(0, 100.0, 40.0, (300.0, 30.0, -1.0), (0.0, 1.0, -3.0)))[2] == 0.0
    for rates in ([[0, 1], [1, 0]], [[0, -1e-3, 0], [1, 0, 0], [1, 0, 0]], [[0, nan, 0], [1, 0, 0], [1, 0, 0]]):
        with pytest.raises(ValueError):
            ms.MultiStateUnit("u", 10.0, 5.0, rates)
    # a row of the rate matrix without an exit: refused when the state can be reached from UP (UP always can), ignored otherwise
    absorbing_down = ms.MultiStateUnit("u", 10.0, 5.0, [[0, .001, .001], [.1, 0, 0], [0, 0, 0]])
    never_fails = ms.MultiStateUnit("u", 10.0, 5.0, [[0, 0, 0], [.1, 0, 0], [.1, 0, 0]])
    absorbing_derated = ms.MultiStateUnit("u", 10.0, 5.0, [[0, .001, 0], [0, 0, 0], [.1, 0, 0]])
    assert absorbing_down.no_exit == (False, False, True) and never_fails.no_exit == (True, False, False)
    for unit, msg in ((absorbing_down, "state DOWN of unit 32 has no exit"), (never_fails, "state UP of unit 32 has no exit"),
                      (absorbing_derated, "state DERATED of unit 32 has no exit")):
        with pytest.raises(ValueError, match=msg):
            ms.run_sequential_multistate(ok + [unit], load, 10, engine=_Untouchable())
        with pytest.raises(ValueError, match="has no exit"):
            ms.run_analytical_multistate([unit], load)
        with pytest.raises(ValueError, match="has no exit"):
            ms.stationary(unit)
    idle_down = ms.MultiStateUnit("u", 10.0, 5.0, [[0, .001, 0], [.1, 0, 0], [0, 0, 0]])      # DOWN has no exit and is never entered
    assert idle_down.no_exit == (False, False, True) and not idle_down.rates[2].any()
    assert ms.stationary(idle_down)[2] == 0.0 and ms.stationary(idle_down)[1] == 10.0 / (1000.0 + 10.0)
    assert ms.run_analytical_multistate([idle_down], hl1.LoadModel(np.array([7.0])), step_size=1.0).lole_hours_yr == pytest.approx(10.0 / 1010.0, rel=1e-12)
    u = ms.MultiStateUnit("u", 10.0, 5.0, [[-9.0, 0.001, 0.003], [0.02, 77.0, 0.02], [0.05, 0.0, 0.0]])      # the diagonal is ignored
    assert u.mean_h == (250.0, 25.0, 20.0) and u.first_p == (0.75, 0.5, 1.0)


def test_derated_rts24():
    fleet, gens = ms.derated_rts24(), hl1.rts24_generators()
    assert len(fleet) == len(gens) == 32
    derated = [u for u in fleet if u.derated_capacity > 0]
    assert sorted(u.capacity for u in derated) == [350.0, 400.0, 400.0] and all(u.derated_capacity == 0.5 * u.capacity for u in derated)
    for u, g in zip(fleet, gens):
        assert u.capacity == g.capacity
        if u.derated_capacity == 0:
            assert (u.mean_h[0], u.mean_h[2], u.first_p[0], u.first_p[2]) == (g.mttf, g.mttr, 1.0, 1.0)
        else:
            assert all(0.0 < p < 1.0 for p in u.first_p) and ms.stationary(u)[1] > 0.01
    assert "ILLUSTRATIVE" in ms.derated_rts24.__doc__
