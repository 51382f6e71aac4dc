"""Tie outages of the HL1 multi-area chronology on the GPU (relmc_hl1_area_tie_outages): the device against the host model
(tests/tools/hl1_tie_model.py) step for step, the exact equalities with the chronology without outage data, the sandwich between perfect
ties and ISOLATED chain-year by chain-year, the exact stationary expectations, split / repeat invariance, the error codes and the Python
surface."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from powersystemsreliabilityassessment_amd import _abi, hl1, hl1_areas

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("hl1_tie_model", os.path.join(ROOT, "tests", "tools", "hl1_tie_model.py"))
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)
AM = M.AM

dp, ip = _abi.c_double_p, _abi.c_int32_p
INF = np.inf


def _arrays(sysm):
    g = [x for a in sysm.areas for x in a.generators]
    return ([len(a.generators) for a in sysm.areas], np.array([x.capacity for x in g]), np.array([x.mttf for x in g]),
            np.array([x.mttr for x in g]), np.stack([np.asarray(a.hourly_load, dtype=np.float64) for a in sysm.areas]))


def _ties(sysm):
    return [(t.from_area - 1, t.to_area - 1, float(t.capacity)) for t in sysm.tie_lines]


def _load(eng, units, cap, mttf, mttr, loads, ties):
    u = np.ascontiguousarray(units, dtype=np.int32)
    arrs = [np.ascontiguousarray(x, dtype=np.float64) for x in (cap, mttf, mttr, loads)]
    tf = np.ascontiguousarray([t[0] for t in ties], dtype=np.int32)
    tt = np.ascontiguousarray([t[1] for t in ties], dtype=np.int32)
    tc = np.ascontiguousarray([t[2] for t in ties], dtype=np.float64)
    eng._check(eng.L.relmc_hl1_area_load(eng._h, u.size, u.ctypes.data_as(ip), *[a.ctypes.data_as(dp) for a in arrs[:3]], arrs[3].shape[-1],
                                         arrs[3].ctypes.data_as(dp), tf.size, tf.ctypes.data_as(ip), tt.ctypes.data_as(ip),
                                         tc.ctypes.data_as(dp)), "relmc_hl1_area_load")
    eng._hl1_area_loaded = None                    # hl1_areas' cache no longer describes the device


def _outages_rc(L, h, kf, kr, n=None):
    if kf is None:
        return L.relmc_hl1_area_tie_outages(h, 0 if n is None else n, None, None)
    kf, kr = np.ascontiguousarray(kf, dtype=np.float64), np.ascontiguousarray(kr, dtype=np.float64)
    return L.relmc_hl1_area_tie_outages(h, kf.size if n is None else n, kf.ctypes.data_as(dp), kr.ctypes.data_as(dp))


def _outages(eng, kf, kr):
    eng._check(_outages_rc(eng.L, eng._h, kf, kr), "relmc_hl1_area_tie_outages")
    eng._hl1_area_loaded = None


def _run(eng, rows, seed, first, n, years, start, policy, flow=M.REFERENCE):
    acc = (_abi.Hl1SeqAcc * rows)()
    yr = np.zeros((n * years, rows, 3))
    eng._check(eng.L.relmc_hl1_area(eng._h, seed, first, n, years, start, policy, flow, acc,
                                    yr.ctypes.data_as(C.POINTER(_abi.Hl1SeqYear))), "relmc_hl1_area")
    return acc, yr


def _assert_model(yr, model, rtol=1e-9):
    np.testing.assert_array_equal(yr[..., 0], model[..., 0])
    np.testing.assert_array_equal(yr[..., 2], model[..., 2])
    np.testing.assert_allclose(yr[..., 1], model[..., 1], rtol=rtol, atol=rtol)


def _acc_tuple(acc):
    return [tuple(getattr(x, f) for f, _ in _abi.Hl1SeqAcc._fields_) for x in acc]


def _fleet5():
    """test_hl1_area.py's 5-area fleet: 100 units in areas of 20, a 1000-hour year, 7 ties of which two are parallel, all failing."""
    cap, mttf, mttr, load = AM.SEQ.fleet100()
    h = np.arange(load.size)
    share = np.array([cap[20 * a:20 * a + 20] @ (mttf / (mttf + mttr))[20 * a:20 * a + 20] for a in range(5)])
    loads = np.stack([share[a] * (0.9 + 0.06 * np.sin(2 * np.pi * (h - 5 * a) / 24.0) + 0.03 * np.sin(2 * np.pi * h / (300.0 + 90 * a)))
                      for a in range(5)])
    ties = [(0, 1, 40.0), (1, 2, 25.5), (2, 3, 60.0), (3, 4, 15.25), (4, 0, 30.0), (0, 2, 10.0), (1, 2, 5.0)]
    kf = np.array([400.0, 650.0, 300.0, 520.0, 480.0, 350.0, 275.0])
    kr = np.array([30.0, 45.0, 25.0, 60.0, 35.0, 40.0, 20.0])
    return [20] * 5, cap, mttf, mttr, loads, ties, kf, kr


def _demo_arrays():
    sysm = hl1_areas.demo_system()
    return _arrays(sysm) + (_ties(sysm),)


FLOWS = [M.REFERENCE, M.MAX_FLOW]


@pytest.mark.gpu
@pytest.mark.parametrize("flow", FLOWS)
def test_device_equals_host_model_demo(engine, flow):
    """The demo system with its tie at 950 h / 50 h, 64 chains x 2 years, both start rules: integers exact, EUE to 1e-9."""
    units, cap, mttf, mttr, loads, ties = _demo_arrays()
    _load(engine, units, cap, mttf, mttr, loads, ties)
    _outages(engine, [950.0], [50.0])
    for start, first in ((M.STATIONARY, 1000), (M.ALL_UP, 7)):
        acc, yr = _run(engine, 3, 11, first, 64, 2, start, M.INTERCONNECTED, flow)
        model = M.interval_model(11, range(first, first + 64), units, cap, mttf, mttr, loads, ties, [950.0], [50.0], 2, start, M.INTERCONNECTED, flow)
        _assert_model(yr, model)
        perfect = AM.interval_model(11, range(first, first + 64), units, cap, mttf, mttr, loads, AM.topology(2, ties), 2, start, M.INTERCONNECTED, flow)
        assert model[:, 1, 0].sum() > perfect[:, 1, 0].sum()              # the outages are seen in these chains
        for r in range(3):
            assert acc[r].years == 128 and acc[r].sum_lole == pytest.approx(yr[:, r, 0].sum(), rel=1e-12)
            assert acc[r].sum_lolf == pytest.approx(yr[:, r, 2].sum(), rel=1e-12)


@pytest.mark.gpu
@pytest.mark.parametrize("flow", FLOWS)
def test_device_equals_host_model_rts96_with_five_lines(engine, flow):
    """RTS-96 with rts96_tie_lines() and the tie MTTFs shortened to ~500 h so that outages occur inside the run; the loads raised so that
    transfers are needed in these few chains."""
    sysm = hl1_areas.rts96_system(tie_outages=True)
    units, cap, mttf, mttr, loads = _arrays(sysm)
    loads = loads * np.array([[1.18], [1.0], [1.22]])
    ties = _ties(sysm)
    kf = np.array([500.0, 450.0, 550.0, 480.0, 520.0])
    kr = np.array([t.mttr for t in sysm.tie_lines]) * 8.0
    _load(engine, units, cap, mttf, mttr, loads, ties)
    _outages(engine, kf, kr)
    _, yr = _run(engine, 4, 5, 3, 16, 2, M.ALL_UP, M.INTERCONNECTED, flow)
    model = M.interval_model(5, range(3, 19), units, cap, mttf, mttr, loads, ties, kf, kr, 2, M.ALL_UP, M.INTERCONNECTED, flow)
    _assert_model(yr, model)
    perfect = AM.interval_model(5, range(3, 19), units, cap, mttf, mttr, loads, sysm.topology_matrix, 2, M.ALL_UP, M.INTERCONNECTED, flow)
    assert model[:, -1, 1].sum() > perfect[:, -1, 1].sum() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("flow", FLOWS)
def test_device_equals_host_model_five_areas(engine, flow):
    """100 units (two per lane) in 5 areas, 7 failing ties (two parallel), a 1000-hour year (windows straddle years), 1 chain x 20 years."""
    units, cap, mttf, mttr, loads, ties, kf, kr = _fleet5()
    _load(engine, units, cap, mttf, mttr, loads, ties)
    _outages(engine, kf, kr)
    for start in (M.STATIONARY, M.ALL_UP):
        _, yr = _run(engine, 6, 3, 2, 1, 20, start, M.INTERCONNECTED, flow)
        model = M.interval_model(3, [2], units, cap, mttf, mttr, loads, ties, kf, kr, 20, start, M.INTERCONNECTED, flow)
        _assert_model(yr, model)
        perfect = AM.interval_model(3, [2], units, cap, mttf, mttr, loads, AM.topology(5, ties), 20, start, M.INTERCONNECTED, flow)
        assert not np.array_equal(model, perfect) and (model[:, :5, 0].sum(0) > 20).all()


@pytest.mark.gpu
def test_exact_equalities_with_the_chronology_without_outage_data(engine):
    units, cap, mttf, mttr, loads, ties, kf, kr = _fleet5()
    nt = len(ties)
    args = (6, 9, 0, 48, 2)
    for start in (M.ALL_UP, M.STATIONARY):
        _load(engine, units, cap, mttf, mttr, loads, ties)
        base = {(p, f): _run(engine, *args, start, p, f) for p, f in ((M.ISOLATED, M.REFERENCE), (M.INTERCONNECTED, M.REFERENCE),
                                                                     (M.INTERCONNECTED, M.MAX_FLOW))}
        same = lambda a, b: np.array_equal(a[1], b[1]) and _acc_tuple(a[0]) == _acc_tuple(b[0])
        # every mttf = inf: the kernel without ties runs
        _outages(engine, np.full(nt, INF), np.full(nt, np.nan))
        for (p, f), b in base.items():
            assert same(_run(engine, *args, start, p, f), b), (start, p, f)
        # failing ties: ISOLATED does not read them, INTERCONNECTED does
        _outages(engine, kf, kr)
        assert same(_run(engine, *args, start, M.ISOLATED, M.REFERENCE), base[(M.ISOLATED, M.REFERENCE)])
        assert not np.array_equal(_run(engine, *args, start, M.INTERCONNECTED, M.MAX_FLOW)[1], base[(M.INTERCONNECTED, M.MAX_FLOW)][1])
        # NULL, NULL and n_ties = 0 remove the data; so does a load
        _outages(engine, None, None)
        assert same(_run(engine, *args, start, M.INTERCONNECTED, M.MAX_FLOW), base[(M.INTERCONNECTED, M.MAX_FLOW)])
        _outages(engine, kf, kr)
        assert _outages_rc(engine.L, engine._h, kf, kr, n=0) == 0
        assert same(_run(engine, *args, start, M.INTERCONNECTED, M.REFERENCE), base[(M.INTERCONNECTED, M.REFERENCE)])
        _outages(engine, kf, kr)
        _load(engine, units, cap, mttf, mttr, loads, ties)
        assert same(_run(engine, *args, start, M.INTERCONNECTED, M.MAX_FLOW), base[(M.INTERCONNECTED, M.MAX_FLOW)])
        # one tie with draws that never fails within the run (the tie kernel runs): all UP at the start it stays UP
        if start == M.ALL_UP:
            _outages(engine, np.where(np.arange(nt) == 3, 1e30, INF), np.ones(nt))
            for f in FLOWS:
                assert same(_run(engine, *args, start, M.INTERCONNECTED, f), base[(M.INTERCONNECTED, f)]), f
            _outages(engine, np.full(nt, 1e30), np.ones(nt))
            for f in FLOWS:
                assert same(_run(engine, *args, start, M.INTERCONNECTED, f), base[(M.INTERCONNECTED, f)]), f
    # failing ties of capacity 0 = INTERCONNECTED with zero-capacity ties
    zero = [(i, j, 0.0) for i, j, _ in ties]
    _load(engine, units, cap, mttf, mttr, loads, zero)
    z0 = _run(engine, *args, M.STATIONARY, M.INTERCONNECTED, M.MAX_FLOW)
    _outages(engine, kf, kr)
    z1 = _run(engine, *args, M.STATIONARY, M.INTERCONNECTED, M.MAX_FLOW)
    assert np.array_equal(z0[1], z1[1]) and _acc_tuple(z0[0]) == _acc_tuple(z1[0])


@pytest.mark.gpu
def test_the_other_hl1_models_are_left_alone(engine):
    gens, load = hl1.rts24_generators(), hl1.rts24_load()
    before = hl1.run_non_sequential_mc(gens, load, 20000, seed=3, engine=engine)
    before_seq = hl1.run_sequential_mc(gens, load, 20, seed=3, engine=engine)
    units, cap, mttf, mttr, loads, ties = _demo_arrays()
    _load(engine, units, cap, mttf, mttr, loads, ties)
    _outages(engine, [950.0], [50.0])
    _run(engine, 3, 1, 0, 32, 1, M.STATIONARY, M.INTERCONNECTED, M.MAX_FLOW)
    after = hl1.run_non_sequential_mc(gens, load, 20000, seed=3, engine=engine)
    after_seq = hl1.run_sequential_mc(gens, load, 20, seed=3, engine=engine)
    assert (before.lole_hours_yr, before.eue_mwh_yr) == (after.lole_hours_yr, after.eue_mwh_yr)
    assert np.array_equal(before.convergence_history, after.convergence_history)
    assert np.array_equal(before_seq.year_lole, after_seq.year_lole) and np.array_equal(before_seq.year_eue, after_seq.year_eue)
    assert np.array_equal(before_seq.year_lolf, after_seq.year_lolf)


@pytest.mark.gpu
def test_sandwich_between_perfect_ties_and_isolated(engine):
    """Chain-year by chain-year under one seed and MAX_FLOW: system EUE(perfect) <= system EUE(failing) <= system EUE(ISOLATED), each up
    to 1e-9 relative: the fleet history is common and the maximum flow is monotone in the capacities."""
    units, cap, mttf, mttr, loads, ties, kf, kr = _fleet5()
    cases = [(units, cap, mttf, mttr, loads, ties, kf, kr, 6)]
    d = _demo_arrays()
    cases.append(d + ([300.0], [40.0], 3))
    for units, cap, mttf, mttr, loads, ties, kf, kr, rows in cases:
        _load(engine, units, cap, mttf, mttr, loads, ties)
        _, perfect = _run(engine, rows, 4, 0, 1000, 1, M.STATIONARY, M.INTERCONNECTED, M.MAX_FLOW)
        _, iso = _run(engine, rows, 4, 0, 1000, 1, M.STATIONARY, M.ISOLATED, M.MAX_FLOW)
        _outages(engine, kf, kr)
        _, fail = _run(engine, rows, 4, 0, 1000, 1, M.STATIONARY, M.INTERCONNECTED, M.MAX_FLOW)
        p, f, i = perfect[:, -1, 1], fail[:, -1, 1], iso[:, -1, 1]
        assert np.all(p <= f * (1 + 1e-9) + 1e-9) and np.all(f <= i * (1 + 1e-9) + 1e-9)
        assert p.sum() < f.sum() < i.sum()


def _mean_se(a, s, s2):
    m = s / a.years
    return m, np.sqrt(max(s2 / a.years - m * m, 0.0) / a.years)


@pytest.mark.gpu
def test_demo_system_against_the_exact_stationary_values_with_a_failing_tie(engine):
    """2e5 one-year chains, stationary start, tie 950 h / 50 h, MAX_FLOW: every row's LOLE and EUE within 4.5 SE of the exact values
    (66.1605 / 1209.3345 / 1213.2357 h/yr, 14579.94 / 184526.09 / 199106.03 MWh/yr), and Area_Poor's perfect-tie LOLE 1095.13 h more than
    4.5 SE away."""
    units, cap, mttf, mttr, loads, ties = _demo_arrays()
    _load(engine, units, cap, mttf, mttr, loads, ties)
    _outages(engine, [950.0], [50.0])
    exact = np.array([[66.1605, 14579.94], [1209.3345, 184526.09], [1213.2357, 199106.03]])
    model = M.joint_stationary_ties(units, cap.astype(int), mttf, mttr, loads, ties, [950.0], [50.0], M.INTERCONNECTED, M.MAX_FLOW)
    np.testing.assert_allclose(model, exact, rtol=1e-3)
    acc, _ = _run(engine, 3, 33, 0, 200000, 1, M.STATIONARY, M.INTERCONNECTED, M.MAX_FLOW)
    for r in range(3):
        for s, s2, e in ((acc[r].sum_lole, acc[r].sum_lole2, model[r, 0]), (acc[r].sum_eue, acc[r].sum_eue2, model[r, 1])):
            m, se = _mean_se(acc[r], s, s2)
            print(f"row {r}: mean {m:.4f} exact {e:.4f} se {se:.4f}")
            assert abs(m - e) < 4.5 * se, (r, m, e, se)
    m, se = _mean_se(acc[1], acc[1].sum_lole, acc[1].sum_lole2)
    assert abs(m - 1095.1342) > 4.5 * se, (m, se)


@pytest.mark.gpu
def test_split_and_repeat_invariance_with_outage_data(engine):
    units, cap, mttf, mttr, loads, ties, kf, kr = _fleet5()
    _load(engine, units, cap, mttf, mttr, loads, ties)
    _outages(engine, kf, kr)
    N, a, Y = 700, 233, 2
    acc, yr = _run(engine, 6, 7, 0, N, Y, M.STATIONARY, M.INTERCONNECTED, M.MAX_FLOW)
    acc1, yr1 = _run(engine, 6, 7, 0, a, Y, M.STATIONARY, M.INTERCONNECTED, M.MAX_FLOW)
    acc2, yr2 = _run(engine, 6, 7, a, N - a, Y, M.STATIONARY, M.INTERCONNECTED, M.MAX_FLOW)
    assert np.array_equal(yr, np.concatenate([yr1, yr2]))
    for r in range(6):
        assert acc[r].years == acc1[r].years + acc2[r].years == N * Y
        for f in ("sum_lole", "sum_eue", "sum_lolf", "sum_lole2", "sum_eue2", "sum_lolf2"):
            assert getattr(acc[r], f) == pytest.approx(getattr(acc1[r], f) + getattr(acc2[r], f), rel=1e-12), f
    acc_r, yr_r = _run(engine, 6, 7, 0, N, Y, M.STATIONARY, M.INTERCONNECTED, M.MAX_FLOW)
    assert np.array_equal(yr, yr_r) and _acc_tuple(acc) == _acc_tuple(acc_r)


@pytest.mark.gpu
def test_error_codes(engine):
    L = engine.L
    h = C.c_void_p()
    assert L.relmc_ctx_create(0, C.byref(h)) == 0
    try:
        assert _outages_rc(L, h, [950.0], [50.0]) == -5                                           # RELMC_ERR_NO_CASE before a load
        assert _outages_rc(L, h, None, None) == -5
        assert _outages_rc(L, None, [950.0], [50.0]) == -1
        units, cap, mttf, mttr, loads, ties, kf, kr = _fleet5()
        u = np.ascontiguousarray(units, dtype=np.int32)
        arrs = [np.ascontiguousarray(x, dtype=np.float64) for x in (cap, mttf, mttr, loads)]

        def load(tl):
            tf = np.ascontiguousarray([t[0] for t in tl], dtype=np.int32)
            tt = np.ascontiguousarray([t[1] for t in tl], dtype=np.int32)
            tc = np.ascontiguousarray([t[2] for t in tl], dtype=np.float64)
            return L.relmc_hl1_area_load(h, u.size, u.ctypes.data_as(ip), *[a.ctypes.data_as(dp) for a in arrs[:3]], arrs[3].shape[-1],
                                         arrs[3].ctypes.data_as(dp), tf.size, tf.ctypes.data_as(ip), tt.ctypes.data_as(ip), tc.ctypes.data_as(dp))

        def run():
            acc = (_abi.Hl1SeqAcc * 6)()
            yr = np.zeros((16 * 2, 6, 3))
            assert L.relmc_hl1_area(h, 5, 0, 16, 2, 1, 1, 1, acc, yr.ctypes.data_as(C.POINTER(_abi.Hl1SeqYear))) == 0
            return yr

        assert load(ties) == 0
        perfect = run()
        assert _outages_rc(L, h, kf, kr) == 0
        ref = run()
        assert not np.array_equal(ref, perfect)
        bad = lambda a, t, v: np.where(np.arange(len(ties)) == t, v, a)
        for v in (0.0, -5.0, np.nan, -np.inf):
            assert _outages_rc(L, h, bad(kf, 4, v), kr) == -1, v
            assert b"tie 4" in L.relmc_last_error(h)
        for v in (0.0, -5.0, np.nan, np.inf, -np.inf):
            assert _outages_rc(L, h, kf, bad(kr, 2, v)) == -1, v
            assert b"tie 2" in L.relmc_last_error(h)
        assert _outages_rc(L, h, kf[:6], kr[:6]) == -1 and _outages_rc(L, h, np.append(kf, 1.0), np.append(kr, 1.0)) == -1   # not the loaded count
        assert _outages_rc(L, h, kf, kr, n=-1) == -1
        assert L.relmc_hl1_area_tie_outages(h, len(ties), kf.ctypes.data_as(dp), None) == -1
        assert L.relmc_hl1_area_tie_outages(h, len(ties), None, kr.ctypes.data_as(dp)) == -1
        assert np.array_equal(run(), ref)                                                         # a refused call changes nothing
        # the mttr of a tie that never fails is not read
        assert _outages_rc(L, h, bad(kf, 1, np.inf), bad(kr, 1, np.nan)) == 0
        assert _outages_rc(L, h, kf, kr) == 0 and np.array_equal(run(), ref)
        # more than 32 ties: the model loads, outage data is refused, and the model runs as before
        many = [(i % 5, (i + 1) % 5, 3.0) for i in range(33)]
        assert load(many) == 0
        before = run()
        assert _outages_rc(L, h, np.full(33, 500.0), np.full(33, 20.0)) == -1
        assert np.array_equal(run(), before)
        assert load(many[:32]) == 0 and _outages_rc(L, h, np.full(32, 500.0), np.full(32, 20.0)) == 0
        assert not np.array_equal(run(), before)
    finally:
        L.relmc_ctx_destroy(h)


@pytest.mark.gpu
def test_python_surface(engine):
    d = hl1_areas.demo_system()
    sysm = hl1_areas.System(d.areas, [hl1_areas.TieLine(1, 2, 200.0, 950.0, 50.0)])
    run = hl1_areas.run_fast_sequential_simulation
    perfect = run(d, hl1_areas.INTERCONNECTED, 256, seed=2, chains=128, start="stationary", flow="max_flow", engine=engine)
    outage = run(sysm, hl1_areas.INTERCONNECTED, 256, seed=2, chains=128, start="stationary", flow="max_flow", engine=engine)
    again = run(d, hl1_areas.INTERCONNECTED, 256, seed=2, chains=128, start="stationary", flow="max_flow", engine=engine)
    assert np.array_equal(perfect.year_indices, again.year_indices)                               # the outage data is cleared again
    units, cap, mttf, mttr, loads = _arrays(sysm)
    m = M.interval_model(2, range(128), units, cap, mttf, mttr, loads, _ties(sysm), [950.0], [50.0], 2, M.STATIONARY, M.INTERCONNECTED, M.MAX_FLOW)
    _assert_model(outage.year_indices, m)
    assert outage.tie_unavailability.tolist() == [0.05] and perfect.tie_unavailability.tolist() == [0.0]
    assert outage.results[1].lole > perfect.results[1].lole and outage.system_eue > perfect.system_eue
    iso = run(sysm, hl1_areas.ISOLATED, 256, seed=2, chains=128, start="stationary", engine=engine)
    iso0 = run(d, hl1_areas.ISOLATED, 256, seed=2, chains=128, start="stationary", engine=engine)
    assert np.array_equal(iso.year_indices, iso0.year_indices)
    rep = hl1_areas.tie_outage_report(perfect, outage)
    assert "PERFECT         | Area_Poor  |" in rep and "FAILING         | SYSTEM     |" in rep and "DIFFERENCE      | Area_Rich  |" in rep
    r96 = run(hl1_areas.rts96_system(tie_outages=True), hl1_areas.INTERCONNECTED, 512, chains=512, start="stationary", flow="max_flow",
              engine=engine)
    assert r96.year_indices.shape == (512, 4, 3) and len(r96.results) == 3
    lines = hl1_areas.rts96_tie_lines()
    np.testing.assert_allclose(r96.tie_unavailability, [t.mttr / (t.mttf + t.mttr) for t in lines], rtol=1e-15)
