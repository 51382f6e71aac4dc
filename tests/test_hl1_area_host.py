"""HL1 multi-area chronology (relmc_hl1_area) without a GPU: the host model's interval form against the reference's loop, the transfer
solve against min-cut enumeration and the package's port, the C ABI's declarations and exports, the Julia constants, and the Python
surface that needs no device."""
import importlib.util
import itertools
import os
import re

import numpy as np
import pytest

from powersystemsreliabilityassessment_amd import _abi, _lib, hl1, hl1_areas

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("hl1_area_model", os.path.join(ROOT, "tests", "tools", "hl1_area_model.py"))
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)


def _arrays(sysm):
    g = [x for a in sysm.areas for x in a.generators]
    return ([len(a.generators) for a in sysm.areas], np.array([x.capacity for x in g]), np.array([x.mttf for x in g]),
            np.array([x.mttr for x in g]), np.stack([np.asarray(a.hourly_load, dtype=np.float64) for a in sysm.areas]))


def _four_areas():
    """4 areas of 3 units, one week of hourly load each, a chain of ties 0-1-2-3 that binds (the reference's break is reached)."""
    h = np.arange(168)
    areas = []
    for a in range(4):
        gens = [hl1.Generator(3 * a + i + 1, c, f, r) for i, (c, f, r) in
                enumerate(((60.0 + 10 * a, 300.0, 40.0), (40.0, 250.0 + 50 * a, 30.0), (25.0, 200.0, 25.0 + 5 * a)))]
        load = np.round(100.0 + 12 * a + 20.0 * np.sin(2 * np.pi * (h - 3 * a) / 24.0), 1)
        areas.append(hl1_areas.Area(a + 1, f"A{a}", gens, load))
    return hl1_areas.System(areas, [hl1_areas.TieLine(1, 2, 30.0), hl1_areas.TieLine(2, 3, 20.0), hl1_areas.TieLine(3, 4, 25.0)])


@pytest.mark.parametrize("start", [M.ALL_UP, M.STATIONARY])
@pytest.mark.parametrize("policy", [M.ISOLATED, M.INTERCONNECTED])
@pytest.mark.parametrize("which,chains,years", [("demo", [0, 5], 2), ("four", [0, 1, 2, 1 << 33], 3)])
def test_interval_form_equals_the_reference_loop(which, chains, years, policy, start):
    """(b) == (a) year by year: loss hours and loss events of every area and of the system exact, EUE to 1e-12."""
    sysm = hl1_areas.demo_system() if which == "demo" else _four_areas()
    units, cap, mttf, mttr, loads = _arrays(sysm)
    a = M.interval_model(5, chains, units, cap, mttf, mttr, loads, sysm.topology_matrix, years, start, policy)
    b = np.concatenate([M.literal_chain(5, c, units, cap, mttf, mttr, loads, sysm.topology_matrix, years, start, policy) for c in chains])
    np.testing.assert_array_equal(a[..., 0], b[..., 0])
    np.testing.assert_array_equal(a[..., 2], b[..., 2])
    np.testing.assert_allclose(a[..., 1], b[..., 1], rtol=1e-12, atol=1e-9)
    assert (a[:, :, 0].sum(0) > 0).all()


def _random_states(rng, n, count, integer):
    T = np.triu(rng.integers(0, 40, (n, n)) * (rng.random((n, n)) < 0.6), 1).astype(float)
    if not integer:
        T = T * rng.uniform(0.5, 1.5, (n, n))
    T = T + T.T
    m = rng.integers(-60, 60, (count, n)).astype(float)
    if not integer:
        m = m + rng.uniform(-1, 1, (count, n))
    return T, m


def _system_of(T):
    n = T.shape[0]
    ties = [hl1_areas.TieLine(i + 1, j + 1, T[i, j]) for i in range(n) for j in range(i + 1, n) if T[i, j] > 0]
    return hl1_areas.System([hl1_areas.Area(i + 1, f"A{i}", [], np.zeros(1)) for i in range(n)], ties)


@pytest.mark.parametrize("n", [2, 3, 5, 8])
def test_solve_curtailment_fast_equals_the_model(n):
    rng = np.random.default_rng(100 + n)
    T, m = _random_states(rng, n, 300, integer=False)
    sysm = _system_of(T)
    np.testing.assert_array_equal(sysm.topology_matrix, T)
    for policy, flow in ((M.ISOLATED, M.REFERENCE), (M.INTERCONNECTED, M.REFERENCE), (M.INTERCONNECTED, M.MAX_FLOW)):
        model = M.solve_batch(m, T, policy, flow)
        port = np.stack([hl1_areas.solve_curtailment_fast(sysm, x, policy, ("reference", "max_flow")[flow]) for x in m])
        np.testing.assert_array_equal(model, port)
    # the literal 1-based transliteration agrees with REFERENCE
    topo = [[0.0] * (n + 1)] + [[0.0] + list(r) for r in T]
    lit = np.array([M._solve_literal(topo, [0.0] + list(x), M.INTERCONNECTED)[1:] for x in m])
    np.testing.assert_array_equal(lit, M.solve_batch(m, T, M.INTERCONNECTED, M.REFERENCE))


@pytest.mark.parametrize("n", [2, 3, 4, 5, 6])
def test_max_flow_is_the_min_cut(n):
    """Integer data: total MAX_FLOW curtailment = total deficit - min over the 2^n cuts of (surplus outside + deficit inside + ties out)."""
    rng = np.random.default_rng(7 + n)
    T, m = _random_states(rng, n, 200, integer=True)
    c = M.solve_batch(m, T, M.INTERCONNECTED, M.MAX_FLOW)
    for x, cx in zip(m, c):
        best = np.inf
        for side in itertools.product((False, True), repeat=n):
            A = np.array(side)
            cut = x[~A & (x > 0)].sum() - x[A & (x < 0)].sum() + T[np.ix_(A, ~A)].sum()
            best = min(best, cut)
        assert cx.sum() == pytest.approx(-x[x < 0].sum() - best, abs=1e-9)
        assert cx.sum() <= M.solve_batch(x[None, :], T, M.INTERCONNECTED, M.REFERENCE).sum() + 1e-9


def test_reference_stops_where_max_flow_goes_on():
    """Ties 0-3 and 2-1, areas 0 and 2 in surplus, 1 and 3 short: area 0 cannot reach area 1, so the reference's loop stops at once."""
    sysm = _system_of(np.array([[0, 0, 0, 80.0], [0, 0, 80.0, 0], [0, 80.0, 0, 0], [80.0, 0, 0, 0]]))
    x = np.array([100.0, -50.0, 100.0, -50.0])
    np.testing.assert_array_equal(hl1_areas.solve_curtailment_fast(sysm, x, hl1_areas.INTERCONNECTED), [0.0, 50.0, 0.0, 50.0])
    np.testing.assert_array_equal(hl1_areas.solve_curtailment_fast(sysm, x, hl1_areas.INTERCONNECTED, "max_flow"), [0.0] * 4)
    np.testing.assert_array_equal(hl1_areas.solve_curtailment_fast(sysm, x, hl1_areas.ISOLATED, "max_flow"), [0.0, 50.0, 0.0, 50.0])
    np.testing.assert_array_equal(M.solve_batch(x[None, :], sysm.topology_matrix, M.INTERCONNECTED, M.MAX_FLOW), [[0.0] * 4])


def test_two_areas_reference_equals_max_flow_and_interconnection_never_hurts():
    rng = np.random.default_rng(3)
    T, m = _random_states(rng, 2, 2000, integer=False)
    T = np.array([[0.0, 37.5], [37.5, 0.0]])
    np.testing.assert_array_equal(M.solve_batch(m, T, M.INTERCONNECTED, M.REFERENCE), M.solve_batch(m, T, M.INTERCONNECTED, M.MAX_FLOW))
    for n in (2, 4, 7):
        T, m = _random_states(np.random.default_rng(n), n, 500, integer=False)
        iso = M.solve_batch(m, T, M.ISOLATED, M.REFERENCE)
        np.testing.assert_array_equal(iso, np.where(m < 0, -m, 0.0))
        for flow in (M.REFERENCE, M.MAX_FLOW):
            assert np.all(M.solve_batch(m, T, M.INTERCONNECTED, flow) <= iso)


def test_exact_stationary_model():
    """(c): ISOLATED rows are each area's own COPT (hl1_seq_model.stationary_year); interconnection lowers every area's LOLE / EUE
    on the demo system, and the system LOLE lies between the largest area LOLE and the sum."""
    sysm = hl1_areas.demo_system()
    units, cap, mttf, mttr, loads = _arrays(sysm)
    iso = M.joint_stationary(units, cap.astype(int), mttf, mttr, loads, sysm.topology_matrix, M.ISOLATED)
    inter = M.joint_stationary(units, cap.astype(int), mttf, mttr, loads, sysm.topology_matrix, M.INTERCONNECTED)
    for a in range(2):
        s = slice(5 * a, 5 * a + 5)
        assert tuple(iso[a]) == pytest.approx(M.SEQ.stationary_year(cap[s].astype(int), mttf[s], mttr[s], loads[a]), rel=1e-12)
    assert np.all(inter[:2] <= iso[:2]) and inter[1, 0] < 0.5 * iso[1, 0]
    assert iso[:2, 0].max() <= iso[2, 0] <= iso[:2, 0].sum()
    assert iso[2, 1] == pytest.approx(iso[:2, 1].sum(), rel=1e-12)


def test_data_helpers():
    ties = hl1_areas.rts96_ties()
    assert [(t.from_area, t.to_area, t.capacity) for t in ties] == [(1, 2, 1175.0), (1, 3, 500.0), (2, 3, 500.0)]
    s = hl1_areas.rts96_system()
    assert [len(a.generators) for a in s.areas] == [32, 32, 32] and s.topology_matrix[0, 1] == 1175.0 == s.topology_matrix[1, 0]
    d = hl1_areas.demo_system()
    assert [a.name for a in d.areas] == ["Area_Rich", "Area_Poor"] and d.topology_matrix.tolist() == [[0.0, 200.0], [200.0, 0.0]]
    assert d.areas[0].hourly_load.size == 8760 and d.areas[1].hourly_load.max() == pytest.approx(1200.0, abs=1e-3)
    par = hl1_areas.System(d.areas, [hl1_areas.TieLine(1, 2, 50.0), hl1_areas.TieLine(2, 1, 25.0)])
    assert par.topology_matrix[0, 1] == 75.0 == par.topology_matrix[1, 0]
    with pytest.raises(ValueError):
        hl1_areas.System(d.areas, [hl1_areas.TieLine(1, 3, 10.0)])


def test_header_declares_and_library_exports_the_multi_area_entry_points():
    hdr = open(os.path.join(ROOT, "include", "relmc.h")).read()
    for s in ("relmc_hl1_area_load", "relmc_hl1_area"):
        assert re.search(r"\b" + s + r"\s*\(", hdr), s
        assert s in _lib.EXPORTS
    defs = dict(re.findall(r"#define (RELMC_(?:AREA_MAX|HL1_AREA_\w+))\s+(\d+)", hdr))
    assert defs == {"RELMC_AREA_MAX": "8", "RELMC_HL1_AREA_ISOLATED": "0", "RELMC_HL1_AREA_INTERCONNECTED": "1",
                    "RELMC_HL1_AREA_FLOW_REFERENCE": "0", "RELMC_HL1_AREA_FLOW_MAX_FLOW": "1"}
    assert (_abi.AREA_MAX, _abi.HL1_AREA_ISOLATED, _abi.HL1_AREA_INTERCONNECTED, _abi.HL1_AREA_FLOW_REFERENCE,
            _abi.HL1_AREA_FLOW_MAX_FLOW) == (8, 0, 1, 0, 1)
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = _lib.load()
    assert hasattr(L, "relmc_hl1_area_load") and hasattr(L, "relmc_hl1_area")


def test_julia_constants_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "relmc.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define (RELMC_(?:AREA_MAX|HL1_AREA_\w+))\s+(\d+)", hdr)}
    jl = open(os.path.join(ROOT, "julia", "RelMC.jl")).read()
    assert int(re.search(r"const AREA_MAX = (\d+)", jl).group(1)) == defs["RELMC_AREA_MAX"]
    pol = dict(re.findall(r":(\w+) => Int32\((\d+)\)", re.search(r"const HL1_AREA_POLICY = Dict\((.*?)\)\s*#", jl).group(1)))
    flow = dict(re.findall(r":(\w+) => Int32\((\d+)\)", re.search(r"const HL1_AREA_FLOW = Dict\((.*?)\)\s*#", jl).group(1)))
    assert {k: int(v) for k, v in pol.items()} == {"isolated": defs["RELMC_HL1_AREA_ISOLATED"], "interconnected": defs["RELMC_HL1_AREA_INTERCONNECTED"]}
    assert {k: int(v) for k, v in flow.items()} == {"reference": defs["RELMC_HL1_AREA_FLOW_REFERENCE"], "max_flow": defs["RELMC_HL1_AREA_FLOW_MAX_FLOW"]}
    assert "relmc_hl1_area_load" in jl and "relmc_hl1_area," in jl


def test_comparison_report():
    """The final table of run_demo (:280-291)."""
    def res(policy, rows):
        return hl1_areas.MultiAreaResult(policy, "reference", [hl1_areas.AreaResult(*r) for r in rows], np.zeros(2), np.zeros(2),
                                         0.0, 0.0, 0.0, 0.0, 0.0)
    iso = res(hl1_areas.ISOLATED, [("Area_Rich", 68.94, 14829.5), ("Area_Poor", 3379.14, 622358.49)])
    inter = res(hl1_areas.INTERCONNECTED, [("Area_Rich", 66.0123, 14566.8), ("Area_Poor", 1095.13, 161482.284)])
    assert hl1_areas.comparison_report(iso, inter) == (
        "\n"
        "=== FINAL COMPARISON (FAST METHOD) ===\n"
        "Policy          | Area       | LOLE (h/yr) | EUE (MWh/yr)\n"
        "------------------------------------------------------------\n"
        "ISOLATED        | Area_Rich  |      68.94  |   14829.50\n"
        "ISOLATED        | Area_Poor  |    3379.14  |  622358.49\n"
        "------------------------------------------------------------\n"
        "INTERCONNECTED  | Area_Rich  |      66.01  |   14566.80\n"
        "INTERCONNECTED  | Area_Poor  |    1095.13  |  161482.28\n")
    assert str(hl1_areas.ISOLATED.name) == "ISOLATED" and int(hl1_areas.INTERCONNECTED) == 1


def test_argument_errors_before_the_device():
    """Every argument error is a ValueError raised before an engine is created (there is no GPU here)."""
    d = hl1_areas.demo_system()
    run = hl1_areas.run_fast_sequential_simulation
    bad_calls = [
        lambda: run(d, hl1_areas.ISOLATED, 10, chains=3),
        lambda: run(d, hl1_areas.ISOLATED, 0),
        lambda: run(d, hl1_areas.ISOLATED, 10, start="cold"),
        lambda: run(d, hl1_areas.INTERCONNECTED, 10, flow="lp"),
        lambda: run(d, 2, 10),
        lambda: run(d, "ISOLATED", 10),
        lambda: run(hl1_areas.System([hl1_areas.Area(i, "x", d.areas[0].generators, d.areas[0].hourly_load) for i in range(9)], []),
                    hl1_areas.ISOLATED, 1),
        lambda: run(hl1_areas.System([d.areas[0], hl1_areas.Area(2, "empty", [], d.areas[1].hourly_load)], []), hl1_areas.ISOLATED, 1),
        lambda: run(hl1_areas.System([d.areas[0], hl1_areas.Area(2, "short", d.areas[1].generators, d.areas[1].hourly_load[:100])], []),
                    hl1_areas.ISOLATED, 1),
        lambda: run(hl1_areas.System(d.areas, [hl1_areas.TieLine(1, 2, -1.0)]), hl1_areas.INTERCONNECTED, 1),
        lambda: run(hl1_areas.System([hl1_areas.Area(1, "big", hl1.rts24_generators() * 5, d.areas[0].hourly_load)], []),
                    hl1_areas.ISOLATED, 1),
        lambda: run(hl1_areas.System([hl1_areas.Area(1, "bad", [hl1.Generator(1, 10.0, 0.0, 5.0)], d.areas[0].hourly_load)], []),
                    hl1_areas.ISOLATED, 1),
        lambda: hl1_areas.solve_curtailment_fast(d, [1.0, -1.0], hl1_areas.INTERCONNECTED, flow="lp"),
        lambda: hl1_areas.solve_curtailment_fast(d, [1.0, -1.0, 0.0], hl1_areas.INTERCONNECTED),
    ]
    for i, call in enumerate(bad_calls):
        with pytest.raises(ValueError):
            call()
