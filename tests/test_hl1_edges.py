"""The four HL1 GPU engines at the edges of their contracts (include/relmc.h): relmc_hl1_nsq against the C oracle and exact sums,
relmc_hl1_seq / relmc_hl1_area / relmc_hl1_plan against their host models (tests/tools/hl1_{seq,area,tie,plan}_model.py) at the unit
counts, year lengths, area counts, topologies, tie counts, index ranges and launch splits where the kernels take paths the other tests
never reach, and the input rule of the four load calls.  The cases are tests/tools/hl1_edge_cases.py's; tests/test_hl1_edges_host.py
ties the host models to the reference loops on the same cases."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from powersystemsreliabilityassessment_amd import _abi, hl1

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", "tools", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


E, SEQ, AREA, TIE, PLAN = (_tool(n) for n in ("hl1_edge_cases", "hl1_seq_model", "hl1_area_model", "hl1_tie_model", "hl1_plan_model"))

dp, ip = _abi.c_double_p, _abi.c_int32_p
POL = [(AREA.ISOLATED, AREA.REFERENCE), (AREA.INTERCONNECTED, AREA.REFERENCE), (AREA.INTERCONNECTED, AREA.MAX_FLOW)]
pytestmark = pytest.mark.gpu


def _ptr(a, t=dp):
    return None if a is None else a.ctypes.data_as(t)


def _f64(*xs):
    return [np.ascontiguousarray(x, dtype=np.float64) for x in xs]


# ---- relmc_hl1_nsq -----------------------------------------------------------------------------------------------------------------
def _nsq_abi(L):
    L.relmc_hl1_load.argtypes = [C.c_void_p, C.c_int32, dp, dp, C.c_int32, dp]
    L.relmc_hl1_nsq.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int64, C.POINTER(hl1.Hl1Acc), dp, dp]


def _nsq_load(L, h, cap, forr, load):
    _nsq_abi(L)
    cap, forr, load = _f64(cap, forr, load)
    return L.relmc_hl1_load(h, cap.size, _ptr(cap), _ptr(forr), load.size, _ptr(load))


def _nsq(eng, cap, forr, load, seed, first, n, want=(True, True)):
    """Load the model, run n iterations; -> (acc, per-iteration loss hours or None, per-iteration EUE or None)."""
    eng._check(_nsq_load(eng.L, eng._h, cap, forr, load), "relmc_hl1_load")
    eng._hl1_loaded = None                                       # hl1.run_non_sequential_mc's cache no longer describes the device
    acc = hl1.Hl1Acc()
    lole, eue = (np.full(n, -1.0) if w else None for w in want)
    eng._check(eng.L.relmc_hl1_nsq(eng._h, seed, first, n, C.byref(acc), _ptr(lole), _ptr(eue)), "relmc_hl1_nsq")
    return acc, lole, eue


def _assert_nsq_oracle(cap, forr, load, seed, first, lole, eue):
    from oracle import coracle
    ol, oe = coracle.hl1_nsq(cap, forr, load, seed, first, lole.size)
    np.testing.assert_array_equal(lole, ol)
    np.testing.assert_allclose(eue, oe, rtol=1e-9, atol=1e-9)
    return ol, oe


@pytest.mark.parametrize("ngen", [1, 3, 4, 5, 63, 64, 65, 127, 128])
def test_nsq_unit_counts_for_extremes_and_ties(engine, ngen):
    """Partial Philox blocks, FOR in {0, 2^-32, 0.5, 1 - 2^-32, 1}, 1 / 2 / 65 / 8760 hours, loads equal to sampled capacities (the
    strict cap < load at exact ties): per-iteration loss hours exact and EUE to 1e-9 against the oracle; loss hours also against the
    numpy restatement of the clamped contract."""
    cap, forr = E.nsq_fleet(ngen)
    seed, first, n = 5 + ngen, 1000, 2048
    up = E.nsq_up(seed, first, n, forr)
    caps = E.unit_order_sum(cap, up)
    assert up[:, 0].all()                                        # FOR 0: always up
    if ngen >= 5:
        assert not up[:, 4].any() and not up[:, 3].any() and up[:, 1].all()   # FOR 1 and 1 - 2^-32: down on these draws; 2^-32: up
    for nhours in (1, 2, 65, 8760):
        load = E.nsq_load(cap, forr, nhours, ties=caps[:3 + nhours // 4])
        acc, lole, eue = _nsq(engine, cap, forr, load, seed, first, n)
        ol, _ = _assert_nsq_oracle(cap, forr, load, seed, first, lole, eue)
        np.testing.assert_array_equal(lole, (np.sort(load)[None, :] > caps[:, None]).sum(1))
        assert acc.n == n and acc.sum_lole == pytest.approx(ol.sum(), rel=1e-12)
        if nhours >= 65:
            assert 0 < ol.sum() < n * nhours                      # the curve straddles the sampled capacities


def test_nsq_grid_stride_index_ranges_and_optional_buffers(engine):
    """n = 3e6 on a 24-hour curve (every thread takes several grid-stride iterations), first_index across 2^32 and at 2^63, and the
    per-iteration buffers one at a time: the same values, the same sums."""
    cap, forr = E.nsq_fleet(33)
    load = E.nsq_load(cap, forr, 24)
    n = 3_000_000
    acc, lole, eue = _nsq(engine, cap, forr, load, 9, 77, n)
    ol, oe = _assert_nsq_oracle(cap, forr, load, 9, 77, lole, eue)
    assert ol.sum() > 0 and acc.n == n
    assert acc.sum_lole == pytest.approx(ol.sum(), rel=1e-12) and acc.sum_eue == pytest.approx(oe.sum(), rel=1e-9)
    assert acc.sum_lole2 == pytest.approx((ol * ol).sum(), rel=1e-12) and acc.sum_eue2 == pytest.approx((oe * oe).sum(), rel=1e-9)
    for first in ((1 << 32) - 3000, (1 << 63) - 3000, 1 << 63):
        _, l, e = _nsq(engine, cap, forr, load, 9, first, 6000)
        _assert_nsq_oracle(cap, forr, load, 9, first, l, e)
    n = 100_000
    base = _nsq(engine, cap, forr, load, 4, 0, n)
    key = lambda a: (a.n, a.sum_lole, a.sum_eue, a.sum_lole2, a.sum_eue2)
    only_l = _nsq(engine, cap, forr, load, 4, 0, n, (True, False))
    only_e = _nsq(engine, cap, forr, load, 4, 0, n, (False, True))
    neither = _nsq(engine, cap, forr, load, 4, 0, n, (False, False))
    assert key(base[0]) == key(only_l[0]) == key(only_e[0]) == key(neither[0])
    assert np.array_equal(only_l[1], base[1]) and np.array_equal(only_e[2], base[2])


def _nsq_flat_curves(engine):
    """(label, device EUE, math.fsum of the per-hour deficits) per scale of eue_scales(), 4096 iterations on 8760 hours."""
    for label, base, spread in E.eue_scales():
        cap, forr, load = E.eue_case(base, spread)
        n = 4096
        _, lole, eue = _nsq(engine, cap, forr, load, 3, 0, n)
        caps = E.unit_order_sum(cap, E.nsq_up(3, 0, n, forr))
        np.testing.assert_array_equal(lole, (load[None, :] > caps[:, None]).sum(1))
        ref = E.exact_eue(caps, load)
        assert (caps == base).sum() > n // 2 and (ref > 0).all()
        yield label, eue, ref


def nsq_eue_rel_errors(engine):
    """Worst per-iteration relative error of relmc_hl1_nsq's EUE on each flat curve."""
    return {label: float(np.max(np.abs(eue - ref) / ref)) for label, eue, ref in _nsq_flat_curves(engine)}


def test_nsq_per_iteration_eue_is_exact_on_flat_curves(engine):
    """Flat curves just above capacity (8760 hours; 1000 + U(0, 1e-3), 3000 + U(0, 1e-6), 1e5 + U(0, 1e-3) MW): EUE to 1e-10 of the
    exact sum, where a plain fp64 suffix sum minus cap * hours loses up to ~1e-6 to cancellation."""
    for label, eue, ref in _nsq_flat_curves(engine):
        np.testing.assert_allclose(eue, ref, rtol=1e-10, atol=1e-12, err_msg=label)


def _last_error(L, h):
    return L.relmc_last_error(h).decode()


def test_nsq_load_rule_and_error_codes(engine):
    """relmc_hl1_load rejects a non-finite capacity, a for_rate outside [0, 1] (NaN included) and a non-finite load, names the unit or
    hour, and keeps the model loaded before; relmc_hl1_nsq(acc = NULL) is RELMC_ERR_INVALID."""
    L = engine.L
    h = C.c_void_p()
    assert L.relmc_ctx_create(0, C.byref(h)) == 0
    try:
        _nsq_abi(L)
        cap, forr = E.nsq_fleet(6)
        load = E.nsq_load(cap, forr, 48)
        assert _nsq_load(L, h, cap, forr, load) == 0
        acc = hl1.Hl1Acc()
        ref = np.zeros(500)
        assert L.relmc_hl1_nsq(h, 2, 0, 500, C.byref(acc), _ptr(ref), None) == 0
        at = lambda x, i, v: np.where(np.arange(x.size) == i, v, x)
        for v in (np.nan, np.inf, -np.inf):
            assert _nsq_load(L, h, at(cap, 4, v), forr, load) == -1 and "unit 4" in _last_error(L, h), v
            assert _nsq_load(L, h, cap, forr, at(load, 31, v)) == -1 and "hour 31" in _last_error(L, h), v
        for v in (np.nan, -1e-300, -0.5, 1.0 + 2.0 ** -52, 2.0, np.inf):
            assert _nsq_load(L, h, cap, at(forr, 2, v), load) == -1 and "unit 2" in _last_error(L, h), v
        for v in (0.0, 1.0):                                      # the closed interval's ends are accepted
            assert _nsq_load(L, h, cap, at(forr, 2, v), load) == 0
        assert _nsq_load(L, h, cap, forr, load) == 0
        assert _nsq_load(L, h, cap, forr, at(load, 0, np.nan)) == -1
        got = np.zeros(500)
        assert L.relmc_hl1_nsq(h, 2, 0, 500, C.byref(acc), _ptr(got), None) == 0 and np.array_equal(got, ref)   # still the last good model
        assert L.relmc_hl1_nsq(h, 2, 0, 500, None, None, None) == -1
        assert L.relmc_hl1_nsq(h, 2, 0, -1, C.byref(acc), None, None) == -1
    finally:
        L.relmc_ctx_destroy(h)


# ---- relmc_hl1_seq -----------------------------------------------------------------------------------------------------------------
def _seq_load(L, h, cap, mttf, mttr, load):
    cap, mttf, mttr, load = _f64(cap, mttf, mttr, load)
    return L.relmc_hl1_seq_load(h, cap.size, _ptr(cap), _ptr(mttf), _ptr(mttr), load.size, _ptr(load))


def _seq(eng, seed, first, n, years, start, records=True):
    acc = _abi.Hl1SeqAcc()
    yr = np.zeros((n * years, 3)) if records else None
    eng._check(eng.L.relmc_hl1_seq(eng._h, seed, first, n, years, start, C.byref(acc), _ptr(yr, C.POINTER(_abi.Hl1SeqYear))), "relmc_hl1_seq")
    return acc, yr


def _assert_records(yr, model):
    np.testing.assert_array_equal(yr[..., 0], model[..., 0])
    np.testing.assert_array_equal(yr[..., 2], model[..., 2])
    np.testing.assert_allclose(yr[..., 1], model[..., 1], rtol=1e-9, atol=1e-9)


def _acc_fields(a):
    return tuple(getattr(a, f) for f, _ in _abi.Hl1SeqAcc._fields_)


@pytest.mark.parametrize("start", [SEQ.ALL_UP, SEQ.STATIONARY])
@pytest.mark.parametrize("nhours", [1, 24, 63, 64, 65, 511, 512, 513])
def test_seq_short_and_window_aligned_years(engine, nhours, start):
    """Years shorter than a 64-lane group (several years close inside one group), at and around the 512-step window, chains of ~1600
    steps (several windows): every record against the interval model."""
    cap, mttf, mttr, load = E.seq_fleet(8, nhours)
    years = E.seq_years(nhours)
    engine._check(_seq_load(engine.L, engine._h, cap, mttf, mttr, load), "relmc_hl1_seq_load")
    engine._hl1_seq_loaded = None
    acc, yr = _seq(engine, 13, 40, 8, years, start)
    model = np.stack(SEQ.interval_model(13, range(40, 48), cap, mttf, mttr, load, years, start), axis=1)
    assert model[:, 0].sum() > 0 and model[:, 2].sum() > 0
    _assert_records(yr, model)
    assert acc.years == 8 * years and acc.sum_lolf == pytest.approx(model[:, 2].sum(), rel=1e-12)


@pytest.mark.parametrize("ngen", [1, 32, 33, 64, 65, 128])
def test_seq_unit_counts_and_transition_extremes(engine, ngen):
    """1 .. 128 units (mask words and both lane slots full at 128), MTTR << 1 h and MTTF >> horizon, a zero-capacity unit and loads equal
    to reachable capacity sums, both start rules, first_chain across 2^32."""
    cap, mttf, mttr, load = E.seq_fleet(ngen, 100)
    engine._check(_seq_load(engine.L, engine._h, cap, mttf, mttr, load), "relmc_hl1_seq_load")
    engine._hl1_seq_loaded = None
    for start, first in ((SEQ.ALL_UP, 0), (SEQ.STATIONARY, (1 << 32) - 4)):
        _, yr = _seq(engine, 3, first, 8, 6, start)
        model = np.stack(SEQ.interval_model(3, range(first, first + 8), cap, mttf, mttr, load, 6, start), axis=1)
        assert model[:, 0].sum() > 0
        _assert_records(yr, model)


def test_seq_two_launches(engine):
    """4300 chains x 1000 years of 24 hours: more than 2^22 records, so two launches.  Chains around the launch boundary against the
    model, the whole call against two calls split there (records bitwise, sums to 1e-12)."""
    cap, mttf, mttr, load = E.seq_fleet(6, 24)
    engine._check(_seq_load(engine.L, engine._h, cap, mttf, mttr, load), "relmc_hl1_seq_load")
    engine._hl1_seq_loaded = None
    N, Y = 4300, 1000
    per = E.RECORD_BUDGET // Y
    assert N * Y > E.RECORD_BUDGET and per < N
    acc, yr = _seq(engine, 8, 0, N, Y, SEQ.STATIONARY)
    w0, w1 = per - 3, per + 3
    model = np.stack(SEQ.interval_model(8, range(w0, w1), cap, mttf, mttr, load, Y, SEQ.STATIONARY), axis=1)
    _assert_records(yr[w0 * Y:w1 * Y], model)
    acc1, yr1 = _seq(engine, 8, 0, per, Y, SEQ.STATIONARY)
    acc2, yr2 = _seq(engine, 8, per, N - per, Y, SEQ.STATIONARY)
    assert np.array_equal(yr[:per * Y], yr1) and np.array_equal(yr[per * Y:], yr2)
    assert acc.years == acc1.years + acc2.years == N * Y
    for f in ("sum_lole", "sum_eue", "sum_lolf", "sum_lole2", "sum_eue2", "sum_lolf2"):
        assert getattr(acc, f) == pytest.approx(getattr(acc1, f) + getattr(acc2, f), rel=1e-12), f
    assert acc.sum_lole == pytest.approx(yr[:, 0].sum(), rel=1e-12)


def test_seq_load_rule(engine):
    L = engine.L
    h = C.c_void_p()
    assert L.relmc_ctx_create(0, C.byref(h)) == 0
    try:
        cap, mttf, mttr, load = E.seq_fleet(5, 30)
        at = lambda x, i, v: np.where(np.arange(x.size) == i, v, x)
        for v in (np.nan, np.inf, -np.inf):
            assert _seq_load(L, h, at(cap, 3, v), mttf, mttr, load) == -1 and "unit 3" in _last_error(L, h), v
            assert _seq_load(L, h, cap, mttf, mttr, at(load, 17, v)) == -1 and "hour 17" in _last_error(L, h), v
        assert L.relmc_hl1_seq(h, 1, 0, 4, 1, 0, C.byref(_abi.Hl1SeqAcc()), None) == -5         # nothing was loaded
        assert _seq_load(L, h, cap, mttf, mttr, load) == 0
        assert _seq_load(L, h, cap, mttf, mttr, at(load, 0, np.nan)) == -1
        assert L.relmc_hl1_seq(h, 1, 0, 4, 1, 0, C.byref(_abi.Hl1SeqAcc()), None) == 0          # the good model stays loaded
    finally:
        L.relmc_ctx_destroy(h)


# ---- relmc_hl1_area ----------------------------------------------------------------------------------------------------------------
def _area_load(L, h, units, cap, mttf, mttr, loads, ties):
    u = np.ascontiguousarray(units, dtype=np.int32)
    cap, mttf, mttr, loads = _f64(cap, mttf, mttr, loads)
    tf, tt = (np.ascontiguousarray([t[i] for t in ties], dtype=np.int32) for i in (0, 1))
    tc = np.ascontiguousarray([t[2] for t in ties], dtype=np.float64)
    return L.relmc_hl1_area_load(h, u.size, _ptr(u, ip), _ptr(cap), _ptr(mttf), _ptr(mttr), loads.shape[-1], _ptr(loads), tf.size,
                                 _ptr(tf, ip), _ptr(tt, ip), _ptr(tc))


def _area(eng, rows, seed, first, n, years, start, policy, flow, records=True):
    acc = (_abi.Hl1SeqAcc * rows)()
    yr = np.zeros((n * years, rows, 3)) if records else None
    eng._check(eng.L.relmc_hl1_area(eng._h, seed, first, n, years, start, policy, flow, acc, _ptr(yr, C.POINTER(_abi.Hl1SeqYear))),
               "relmc_hl1_area")
    return acc, yr


@pytest.mark.parametrize("policy,flow", POL)
@pytest.mark.parametrize("topo", ["complete", "path", "star", "two_components", "zero_ties"])
def test_area_eight_areas_topologies(engine, topo, policy, flow):
    """RELMC_AREA_MAX = 8 areas (the largest dynamic LDS), 128 units split 1/1/30/40/20/10/25/1, on a complete graph with parallel ties,
    a 7-hop path, a star, two components and zero-capacity ties; first_chain across 2^32: every record against the model."""
    units, cap, mttf, mttr, loads = E.area_fleet8()
    ties = E.topologies8()[topo]
    engine._check(_area_load(engine.L, engine._h, units, cap, mttf, mttr, loads, ties), "relmc_hl1_area_load")
    engine._hl1_area_loaded = None
    T = AREA.topology(8, ties)
    for start, first in ((AREA.STATIONARY, 0), (AREA.ALL_UP, (1 << 32) - 2)):
        acc, yr = _area(engine, 9, 21, first, 8, 2, start, policy, flow)
        model = AREA.interval_model(21, range(first, first + 8), units, cap, mttf, mttr, loads, T, 2, start, policy, flow)
        assert model[:, 8, 0].sum() > 0
        _assert_records(yr, model)
        for r in range(9):
            assert acc[r].years == 16 and acc[r].sum_lole == pytest.approx(model[:, r, 0].sum(), rel=1e-12)


@pytest.mark.parametrize("flow", [AREA.REFERENCE, AREA.MAX_FLOW])
@pytest.mark.parametrize("start", [AREA.ALL_UP, AREA.STATIONARY])
@pytest.mark.parametrize("ngen", [64, 65])
@pytest.mark.parametrize("nhours", [511, 512, 513])
def test_area_tie_slot_at_the_window_edges(engine, nhours, ngen, start, flow):
    """The tie slot of the chronology with all 32 tie lanes busy (MTTR << 1 h, MTTF of a few hours, mttf = inf and 1e30, parallel and
    reversed ties), with one unit slot (64 units) and two (65), on years at and around the 512-step window, 4 chains of ~2000 steps
    (year boundaries inside 64-step groups): every record against hl1_tie_model."""
    units, cap, mttf, mttr, loads, ties, kf, kr = E.area_tie_edges(ngen, nhours)
    years = E.seq_years(nhours)
    engine._check(_area_load(engine.L, engine._h, units, cap, mttf, mttr, loads, ties), "relmc_hl1_area_load")
    kf_, kr_ = _f64(kf, kr)
    engine._check(engine.L.relmc_hl1_area_tie_outages(engine._h, kf_.size, _ptr(kf_), _ptr(kr_)), "relmc_hl1_area_tie_outages")
    engine._hl1_area_loaded = None
    pol = (years, start, AREA.INTERCONNECTED, flow)
    _, yr = _area(engine, 5, 17, 2, 4, *pol)
    model = TIE.interval_model(17, range(2, 6), units, cap, mttf, mttr, loads, ties, kf, kr, *pol)
    perfect = AREA.interval_model(17, range(2, 6), units, cap, mttf, mttr, loads, AREA.topology(4, ties), *pol)
    assert model[:, 4, 0].sum() > perfect[:, 4, 0].sum() > 0      # the chains need transfers, and the outages are seen in them
    _assert_records(yr, model)


def test_area_two_launches(engine):
    """2 areas, 4300 chains x 1000 years of 24 hours (two launches): chains around the boundary against the model, the whole call
    against two calls split there."""
    cap, mttf, mttr, load = E.seq_fleet(12, 24)
    units = [5, 7]
    loads = np.stack([load * 0.45, load * 0.55])
    ties = [(0, 1, 20.0)]
    engine._check(_area_load(engine.L, engine._h, units, cap, mttf, mttr, loads, ties), "relmc_hl1_area_load")
    engine._hl1_area_loaded = None
    N, Y = 4300, 1000
    per = E.RECORD_BUDGET // Y
    pol = (AREA.STATIONARY, AREA.INTERCONNECTED, AREA.MAX_FLOW)
    acc, yr = _area(engine, 3, 6, 0, N, Y, *pol)
    w0, w1 = per - 2, per + 2
    model = AREA.interval_model(6, range(w0, w1), units, cap, mttf, mttr, loads, AREA.topology(2, ties), Y, *pol)
    assert model[:, 2, 0].sum() > 0
    _assert_records(yr[w0 * Y:w1 * Y], model)
    acc1, yr1 = _area(engine, 3, 6, 0, per, Y, *pol)
    acc2, yr2 = _area(engine, 3, 6, per, N - per, Y, *pol)
    assert np.array_equal(yr[:per * Y], yr1) and np.array_equal(yr[per * Y:], yr2)
    del yr, yr1, yr2
    for r in range(3):
        assert acc[r].years == N * Y
        for f in ("sum_lole", "sum_eue", "sum_lolf", "sum_lole2", "sum_eue2", "sum_lolf2"):
            assert getattr(acc[r], f) == pytest.approx(getattr(acc1[r], f) + getattr(acc2[r], f), rel=1e-12), (r, f)


def test_area_load_rule(engine):
    L = engine.L
    h = C.c_void_p()
    assert L.relmc_ctx_create(0, C.byref(h)) == 0
    try:
        units, cap, mttf, mttr, loads = E.area_fleet8(nhours=30)
        ties = E.topologies8()["path"]
        at = lambda x, i, v: np.where(np.arange(x.size) == i, v, x)
        for v in (np.nan, np.inf, -np.inf):
            assert _area_load(L, h, units, at(cap, 100, v), mttf, mttr, loads, ties) == -1 and "unit 100" in _last_error(L, h), v
            bad = loads.copy()
            bad[6, 29] = v
            assert _area_load(L, h, units, cap, mttf, mttr, bad, ties) == -1 and "area 6 hour 29" in _last_error(L, h), v
        assert _area_load(L, h, units, cap, mttf, mttr, loads, ties) == 0
        bad = loads.copy()
        bad[0, 0] = np.nan
        assert _area_load(L, h, units, cap, mttf, mttr, bad, ties) == -1
        assert L.relmc_hl1_area(h, 1, 0, 2, 1, 0, 1, 1, (_abi.Hl1SeqAcc * 9)(), None) == 0        # the good model stays loaded
    finally:
        L.relmc_ctx_destroy(h)


# ---- relmc_hl1_plan ----------------------------------------------------------------------------------------------------------------
def _plan_load(L, h, data, sigma):
    cap, forr, limit, load = _f64(data[0], data[1], data[4], data[5])
    st, wk = (np.ascontiguousarray(x, dtype=np.int32) for x in (data[2], data[3]))
    return L.relmc_hl1_plan_load(h, cap.size, _ptr(cap), _ptr(forr), _ptr(st, ip), _ptr(wk, ip), _ptr(limit), load.size, _ptr(load), sigma)


def _plan(eng, seed, first, n, nhours, n_elu, records=True):
    acc = _abi.Hl1SeqAcc()
    yr = np.zeros((n, 3)) if records else None
    hours = np.full(nhours, -1, dtype=np.int64)
    elu = np.zeros((n, max(n_elu, 1))) if records else None
    eng._check(eng.L.relmc_hl1_plan(eng._h, seed, first, n, C.byref(acc), _ptr(yr, C.POINTER(_abi.Hl1SeqYear)), _ptr(hours, _abi.c_int64_p),
                                    _ptr(elu)), "relmc_hl1_plan")
    return acc, yr, hours, None if elu is None else elu[:, :n_elu]


def _plan_check(eng, data, sigma, seed, first, n):
    eng._check(_plan_load(eng.L, eng._h, data, sigma), "relmc_hl1_plan_load")
    eng._hl1_plan_loaded = None
    n_elu = int(np.isfinite(data[4]).sum())
    acc, yr, hours, elu = _plan(eng, seed, first, n, len(data[5]), n_elu)
    lole, eue, lolf, counts, energy, ties = PLAN.model(seed, range(first, first + n), *data, sigma)
    assert ties == 0
    np.testing.assert_array_equal(yr[:, 0], lole)
    np.testing.assert_array_equal(yr[:, 2], lolf)
    np.testing.assert_array_equal(hours, counts)
    np.testing.assert_allclose(yr[:, 1], eue, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(elu, energy, rtol=1e-9, atol=1e-9)
    assert acc.years == n and acc.sum_lole == pytest.approx(lole.sum(), rel=1e-12)
    return yr, hours, elu


@pytest.mark.parametrize("binding", [True, False])
def test_plan_eight_elus_week_53(engine, binding):
    """8 ELUs (every unrolled slot live), binding and not, 8760 hours (week 53), maintenance windows past the year's end and in week 53."""
    data, sigma = E.plan_fleet(14, n_elu=8, binding=binding)
    yr, hours, elu = _plan_check(engine, data, sigma, 7, 100, 64)
    assert hours[8736:].sum() > 0 and yr[:, 0].sum() > 0
    lim = data[4][-8:]
    if binding:
        assert (elu >= lim[None, :] - 1e-9).any(axis=0).all()      # every slot reaches its limit in some year
    else:
        assert (elu > 0).any(axis=0).all() and (elu < lim[None, :]).all()


@pytest.mark.parametrize("ngen", [1, 2, 3, 6, 7, 128])
def test_plan_unit_counts(engine, ngen):
    """Block 0 carries the two LFU words and units 0 and 1, block b units 4b - 2 .. 4b + 1: 1 .. 128 units, 8760 hours, LFU on and
    (ngen = 6) sigma = 0, ELUs where the fleet has room for them."""
    data, sigma = E.plan_fleet(ngen, n_elu=min(2, ngen - 1))
    _plan_check(engine, data, 0.0 if ngen == 6 else sigma, 11, 5, 16 if ngen == 128 else 40)


def test_plan_partial_waves(engine):
    """n_years not a multiple of 64: the lanes without a year are outside the ballot of the hour counts."""
    data, sigma = E.plan_fleet(9, nhours=336, n_elu=2)
    for n in (1, 65, 257):
        _plan_check(engine, data, sigma, 2, 9, n)


def test_plan_two_launches_share_the_hour_counts(engine):
    """2^20 + 100 years of 24 hours: two launches add into one hour-count buffer cleared once per call.  The counts are the split calls'
    sums, a repeated call overwrites them, the records equal the split calls' and the model's around the boundary."""
    data, sigma = E.plan_fleet(6, nhours=24, n_elu=1)
    engine._check(_plan_load(engine.L, engine._h, data, sigma), "relmc_hl1_plan_load")
    engine._hl1_plan_loaded = None
    per = 1 << 20
    N = per + 100
    acc, yr, hours, _ = _plan(engine, 4, 0, N, 24, 1)
    acc1, yr1, h1, _ = _plan(engine, 4, 0, per, 24, 1)
    acc2, yr2, h2, _ = _plan(engine, 4, per, N - per, 24, 1)
    assert np.array_equal(hours, h1 + h2) and hours.sum() == yr[:, 0].sum() > 0
    assert np.array_equal(yr[:per], yr1) and np.array_equal(yr[per:], yr2)
    assert acc.sum_lole == pytest.approx(acc1.sum_lole + acc2.sum_lole, rel=1e-12) and acc.years == N
    _, _, again, _ = _plan(engine, 4, 0, N, 24, 1, records=False)
    assert np.array_equal(again, hours)
    w0, w1 = per - 70, per + 70
    lole, eue, lolf, _, _, ties = PLAN.model(4, range(w0, w1), *data, sigma)
    assert ties == 0
    np.testing.assert_array_equal(yr[w0:w1, 0], lole)
    np.testing.assert_array_equal(yr[w0:w1, 2], lolf)
    np.testing.assert_allclose(yr[w0:w1, 1], eue, rtol=1e-9, atol=1e-9)


def test_plan_load_rule(engine):
    L = engine.L
    h = C.c_void_p()
    assert L.relmc_ctx_create(0, C.byref(h)) == 0
    try:
        data, sigma = E.plan_fleet(5, nhours=40, n_elu=1)
        at = lambda x, i, v: np.where(np.arange(x.size) == i, v, x)
        with_ = lambda k, v: [v if j == k else d for j, d in enumerate(data)]
        for v in (np.nan, np.inf, -np.inf):
            assert _plan_load(L, h, with_(0, at(data[0], 3, v)), sigma) == -1 and "unit 3" in _last_error(L, h), v
            assert _plan_load(L, h, with_(5, at(data[5], 39, v)), sigma) == -1 and "hour 39" in _last_error(L, h), v
        for v in (np.nan, -0.25, 1.5):
            assert _plan_load(L, h, with_(1, at(data[1], 1, v)), sigma) == -1 and "unit 1" in _last_error(L, h), v
        assert _plan_load(L, h, data, sigma) == 0
        assert _plan_load(L, h, with_(5, at(data[5], 0, np.nan)), sigma) == -1
        assert L.relmc_hl1_plan(h, 1, 0, 3, C.byref(_abi.Hl1SeqAcc()), None, None, None) == 0      # the good model stays loaded
    finally:
        L.relmc_ctx_destroy(h)
