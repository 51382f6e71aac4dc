"""The HL1 host models at the edges tests/test_hl1_edges.py runs the device on (no GPU): the interval / vectorised forms against the
literal transliterations of the reference loops (hl1_seq_model.literal_chain, hl1_area_model.literal_chain, hl1_tie_model.literal_chain,
hl1_plan_model.literal_year),
MAX_FLOW against min-cut enumeration on 7 and 8 areas and the edge topologies, and the oracle's clamped HL1 threshold against a numpy
restatement of the contract."""
import importlib.util
import itertools
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", "tools", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


E, SEQ, AREA, TIE, PLAN = (_tool(n) for n in ("hl1_edge_cases", "hl1_seq_model", "hl1_area_model", "hl1_tie_model", "hl1_plan_model"))


def _assert_same(a, b):
    np.testing.assert_array_equal(a[..., 0], b[..., 0])
    np.testing.assert_array_equal(a[..., 2], b[..., 2])
    np.testing.assert_allclose(a[..., 1], b[..., 1], rtol=1e-12, atol=1e-9)


@pytest.mark.parametrize("start", [SEQ.ALL_UP, SEQ.STATIONARY])
@pytest.mark.parametrize("ngen,nhours,years", [(8, 1, 300), (8, 24, 20), (8, 63, 8), (33, 65, 4), (5, 513, 2), (1, 24, 10)])
def test_seq_interval_form_equals_the_hour_loop_at_the_edges(ngen, nhours, years, start):
    """Years shorter than 64 steps, MTTR << 1 h, MTTF >> horizon, a zero-capacity unit and loads equal to capacity sums."""
    cap, mttf, mttr, load = E.seq_fleet(ngen, nhours)
    chains = [3, (1 << 32) + 1]
    a = np.stack(SEQ.interval_model(2, chains, cap, mttf, mttr, load, years, start), axis=1)
    b = np.concatenate([np.stack(SEQ.literal_chain(2, c, cap, mttf, mttr, load, years, start), axis=1) for c in chains])
    _assert_same(a, b)
    assert a[:, 0].sum() > 0 and a[:, 2].sum() > 0


@pytest.mark.parametrize("policy", [AREA.ISOLATED, AREA.INTERCONNECTED])
@pytest.mark.parametrize("topo", ["complete", "path", "two_components", "zero_ties"])
def test_area_interval_form_equals_the_reference_loop_on_8_areas(topo, policy):
    """8 areas of 1 .. 40 units on the complete graph with parallel ties, the 7-hop path, two components and zero ties."""
    units, cap, mttf, mttr, loads = E.area_fleet8(nhours=24)
    T = AREA.topology(8, E.topologies8()[topo])
    chains = [0, 1, 2, 3, (1 << 32) + 9]
    a = AREA.interval_model(4, chains, units, cap, mttf, mttr, loads, T, 2, AREA.STATIONARY, policy)
    b = np.concatenate([AREA.literal_chain(4, c, units, cap, mttf, mttr, loads, T, 2, AREA.STATIONARY, policy) for c in chains])
    _assert_same(a, b)
    assert a[:, 8, 0].sum() > 0


@pytest.mark.parametrize("flow", [AREA.REFERENCE, AREA.MAX_FLOW])
@pytest.mark.parametrize("start", [AREA.ALL_UP, AREA.STATIONARY])
@pytest.mark.parametrize("ngen", [64, 65])
@pytest.mark.parametrize("nhours", [511, 512, 513])
def test_tie_interval_form_equals_the_hour_loop_at_the_window_edges(nhours, ngen, start, flow):
    """test_hl1_edges.py's tie cases (32 ties with MTTR << 1 h, MTTF of a few hours, mttf = inf and 1e30; 64 and 65 units in 4 areas;
    years around 512 hours): the expected values of the device test come from the hour loop as well."""
    units, cap, mttf, mttr, loads, ties, kf, kr = E.area_tie_edges(ngen, nhours)
    pol = (E.seq_years(nhours), start, AREA.INTERCONNECTED, flow)
    chains = range(2, 6)
    a = TIE.interval_model(17, chains, units, cap, mttf, mttr, loads, ties, kf, kr, *pol)
    b = np.concatenate([TIE.literal_chain(17, c, units, cap, mttf, mttr, loads, ties, kf, kr, *pol) for c in chains])
    _assert_same(a, b)
    assert a[:, 4, 0].sum() > 0


@pytest.mark.parametrize("ngen,n_elu,binding", [(1, 0, True), (2, 1, True), (3, 2, True), (10, 8, True), (10, 8, False)])
def test_plan_model_equals_the_literal_year_in_week_53(ngen, n_elu, binding):
    """8760 hours (week 53), maintenance past the year's end and in week 53, 0 .. 8 ELUs: every year, hour and ELU energy."""
    data, sigma = E.plan_fleet(ngen, n_elu=n_elu, binding=binding)
    years = [0, (1 << 32) + 5]
    lole, eue, lolf, counts, energy, ties = PLAN.model(6, years, *data, sigma)
    assert ties == 0
    hours = np.zeros(8760, dtype=np.int64)
    for i, y in enumerate(years):
        l, e, f, loss_hours, elu = PLAN.literal_year(6, y, *data, sigma)
        assert (lole[i], lolf[i]) == (l, f) and eue[i] == pytest.approx(e, rel=1e-12)
        np.testing.assert_allclose(energy[i], elu, rtol=1e-12, atol=1e-9)
        hours[loss_hours] += 1
    np.testing.assert_array_equal(counts, hours)
    lo, hi = PLAN.maintenance_hours(data[2], data[3], 8760)
    assert (hi == 8760).any() and (ngen == 1 or (lo == 8736).any())   # windows run past the end and start in week 53


def _min_cut_check(T, m):
    n = T.shape[0]
    c = AREA.solve_batch(m, T, AREA.INTERCONNECTED, AREA.MAX_FLOW)
    ref = AREA.solve_batch(m, T, AREA.INTERCONNECTED, AREA.REFERENCE)
    sides = np.array(list(itertools.product((False, True), repeat=n)))
    for x, cx, rx in zip(m, c, ref):
        cuts = [x[~A & (x > 0)].sum() - x[A & (x < 0)].sum() + T[np.ix_(A, ~A)].sum() for A in sides]
        assert cx.sum() == pytest.approx(-x[x < 0].sum() - min(cuts), abs=1e-9)
        assert cx.sum() <= rx.sum() + 1e-9


@pytest.mark.parametrize("n", [7, 8])
def test_max_flow_is_the_min_cut_on_7_and_8_areas(n):
    """test_hl1_area_host.test_max_flow_is_the_min_cut extended: random integer ties and margins on 7 and 8 areas."""
    rng = np.random.default_rng(70 + n)
    T = np.triu(rng.integers(0, 40, (n, n)) * (rng.random((n, n)) < 0.6), 1).astype(float)
    T = T + T.T
    _min_cut_check(T, rng.integers(-60, 60, (60, n)).astype(float))


@pytest.mark.parametrize("topo", ["complete", "path", "star", "two_components", "zero_ties"])
def test_max_flow_is_the_min_cut_on_the_edge_topologies(topo):
    """The 8-area topologies of the device tests, integer-rounded, with margins that put surplus and deficit at the path's two ends."""
    T = np.round(AREA.topology(8, E.topologies8()[topo]))
    rng = np.random.default_rng(len(topo))
    m = rng.integers(-60, 60, (60, 8)).astype(float)
    m[:20, 0] = 200.0
    m[:20, 7] = -150.0
    m[:20, 1:7] = 0.0
    _min_cut_check(T, m)


@pytest.mark.parametrize("for_rate", [0.0, 1.0])
def test_oracle_threshold_is_clamped(for_rate):
    """orc_hl1_nsq at FOR 0 and 1 (and 2^-32, 1 - 2^-32 alongside) against the clamped contract restated in numpy."""
    from oracle import coracle
    cap = np.array([10.5, 20.25, 30.125, 40.0625, 50.5, 7.75])
    forr = np.array([for_rate, 2.0 ** -32, 0.5, 1.0 - 2.0 ** -32, for_rate, 0.25])
    load = np.array([5.0, 50.0, 100.0, 120.0, 158.0, 159.1875, 170.0])
    n = 20000
    lole, eue = coracle.hl1_nsq(cap, forr, load, 3, (1 << 32) - 7, n)
    up = E.nsq_up(3, (1 << 32) - 7, n, forr)
    assert up[:, 0].all() == (for_rate == 0.0) and up[:, 4].any() == (for_rate == 0.0)
    caps = E.unit_order_sum(cap, up)
    np.testing.assert_array_equal(lole, (load[None, :] > caps[:, None]).sum(1))
    np.testing.assert_allclose(eue, np.where(load[None, :] > caps[:, None], load[None, :] - caps[:, None], 0.0).sum(1), rtol=1e-12, atol=1e-12)
    np.testing.assert_array_equal(E.nsq_thresholds([0.0, 1.0, 2.0 ** -32, 1.0 - 2.0 ** -32]), [0, 2 ** 32 - 1, 1, 2 ** 32 - 1])
