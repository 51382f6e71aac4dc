"""Planned maintenance on the HL1 sequential chronology on the GPU (relmc_hl1_maint_load, relmc_hl1_maint_seq): the empty schedule against
relmc_hl1_seq and the sweep bit for bit, whole-year windows against the sweep's withheld fleet bit for bit, window edges against the host
model (tests/tools/hl1_maint_model.py), independence of the schedules, split / chunk / repeat invariance, nested schedules, the chain
counts, the error codes, the exact answers of run_analytical_maintenance and the paired comparison of hl1_maintenance.py."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from powersystemsreliabilityassessment_amd import _abi, hl1, hl1_maintenance as hm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("hl1_maint_model", os.path.join(ROOT, "tests", "tools", "hl1_maint_model.py"))
MM = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(MM)
M = MM.SEQ

dp = _abi.c_double_p
YP = C.POINTER(_abi.Hl1SeqYear)
ACC_FIELDS = [f for f, _ in _abi.Hl1SeqAcc._fields_]
WH = (3, 40, 70, 99)                 # fleet100: both slots of a lane, all four mask words

# fleet100(513), H = 513: a 64-step group ends with hour 63 in chain year 0 (one hour later every year), the LDS window with hour 511.
# Edges on the group boundary and one step either side, on the window boundary (step 512 / 513), at hour 0 and hour H - 1, a window that
# wraps the year's end, windows of one hour and of H hours, overlapping windows of one unit, units of both lane slots.
S513 = [
    [],
    [(3, 63, 2), (40, 64, 1), (70, 65, 447), (99, 512, 1)],
    [(3, 0, 513), (70, 0, 1), (99, 511, 2), (40, 62, 1)],
    [(40, 500, 100), (99, 512, 2), (70, 100, 200), (70, 250, 120), (3, 64, 449)],
    [(k, 0, 513) for k in WH],
    [(70, 65, 447)],
    [(3, 63, 1), (3, 64, 1), (3, 65, 1), (99, 0, 64), (64, 511, 1), (63, 512, 1)],
    [(k, 200, 150) for k in range(0, 100, 7)],
]
# the six-unit fleet, H = 168 (shorter than a window, no multiple of 64): step 513 is hour 8 of chain year 3
S168 = [
    [],
    [(0, 63, 2), (1, 64, 1), (2, 0, 168), (3, 167, 1)],
    [(4, 160, 20), (5, 0, 1), (1, 100, 30), (1, 120, 30), (5, 7, 2), (0, 8, 160)],
    [(0, 65, 1), (3, 62, 1), (2, 167, 2)],
]


def _rts24():
    gens, load = hl1.rts24_generators(), hl1.rts24_load()
    return (np.array([g.capacity for g in gens]), np.array([g.mttf for g in gens]), np.array([g.mttr for g in gens]), load.hourly_load)


def _fleet(name):
    return _rts24() if name == "rts24" else M.small_fleet() if name == "small" else M.fleet100(int(name))


def _load(eng, cap, mttf, mttr, load, h=None):
    arrs = [np.ascontiguousarray(x, dtype=np.float64) for x in (cap, mttf, mttr, load)]
    rc = eng.L.relmc_hl1_seq_load(h or eng._h, arrs[0].size, *[a.ctypes.data_as(dp) for a in arrs[:3]], arrs[3].size, arrs[3].ctypes.data_as(dp))
    if h is None:
        eng._check(rc, "relmc_hl1_seq_load")
        eng._hl1_seq_loaded = None                 # hl1's cache no longer describes the device
    return rc


def _seq(eng, seed, first, n, years, start):
    acc = _abi.Hl1SeqAcc()
    yr = np.zeros((n * years, 3))
    eng._check(eng.L.relmc_hl1_seq(eng._h, seed, first, n, years, start, C.byref(acc), yr.ctypes.data_as(YP)), "relmc_hl1_seq")
    return acc, yr


def _mask(units):
    m = (C.c_uint32 * 4)()
    for k in units:
        m[k >> 5] |= 1 << (k & 31)
    return m


def _sweep_level(eng, seed, first, n, years, start, scale, shift, fleet, withheld=None):
    arr = (_abi.Hl1SweepLevel * 1)(_abi.Hl1SweepLevel(scale, shift, fleet, 0))
    acc = (_abi.Hl1SeqAcc * 1)()
    yr = np.zeros((n * years, 3))
    eng._check(eng.L.relmc_hl1_seq_sweep(eng._h, seed, first, n, years, start, 1, arr, None if withheld is None else _mask(withheld), acc,
                                         yr.ctypes.data_as(YP)), "relmc_hl1_seq_sweep")
    return acc[0], yr


def _windows(schedules):
    flat = [_abi.Hl1MaintWindow(j, *w) for j, s in enumerate(schedules) for w in s]
    return (_abi.Hl1MaintWindow * max(len(flat), 1))(*flat), len(flat)


def _maint_load(eng, schedules, h=None):
    arr, n = _windows(schedules)
    rc = eng.L.relmc_hl1_maint_load(h or eng._h, len(schedules), n, arr if n else None)
    if h is None:
        eng._check(rc, "relmc_hl1_maint_load")
    return rc


def _maint(eng, seed, first, n, years, start, ns, scale=1.0, shift=0.0, want_years=True, h=None):
    """-> (acc[ns], yr[ns, n * years, 3], rc) under the loaded schedules."""
    acc = (_abi.Hl1SeqAcc * max(ns, 1))()
    yr = np.zeros((max(ns, 1), max(n * years, 0), 3))
    rc = eng.L.relmc_hl1_maint_seq(h or eng._h, seed, first, n, years, start, scale, shift, acc, yr.ctypes.data_as(YP) if want_years else None)
    if h is None:
        eng._check(rc, "relmc_hl1_maint_seq")
    return acc, yr, rc


def _run(eng, schedules, seed, first, n, years, start, *scale_shift, **kw):
    _maint_load(eng, schedules)
    return _maint(eng, seed, first, n, years, start, len(schedules), *scale_shift, **kw)


def _acc_tuple(a):
    return tuple(getattr(a, f) for f in ACC_FIELDS)


@pytest.mark.gpu
@pytest.mark.parametrize("start", [M.ALL_UP, M.STATIONARY])
@pytest.mark.parametrize("fleet,n,years", [("rts24", 64, 3), ("513", 16, 5)])
def test_empty_schedule_is_the_sequential_kernel_bitwise(engine, fleet, n, years, start):
    """Consequence 1: a schedule without windows gives relmc_hl1_seq's year records at (1, 0) and the sweep's level (scale, shift, fleet 0)
    at any scale and shift, bit for bit, alone (one-schedule kernel) and beside another schedule (the wider kernels); acc sums its years."""
    _load(engine, *_fleet(fleet))
    _, ref = _seq(engine, 11, 2, n, years, start)
    _, lvl = _sweep_level(engine, 11, 2, n, years, start, 1.0, 0.0, 0)
    _, lvl2 = _sweep_level(engine, 11, 2, n, years, start, 1.07, 33.25, 0)
    assert ref[:, 0].sum() > 0 and lvl2[:, 0].sum() > ref[:, 0].sum()
    other = [(1, 100, 300)]
    for sched, j in (([[]], 0), ([[], other], 0), ([other, other, []], 2)):
        acc, yr, _ = _run(engine, sched, 11, 2, n, years, start)
        assert yr[j].tobytes() == ref.tobytes() == lvl.tobytes(), (len(sched), j)
        acc2, yr2, _ = _maint(engine, 11, 2, n, years, start, len(sched), 1.07, 33.25)
        assert yr2[j].tobytes() == lvl2.tobytes(), (len(sched), j)
        assert acc[j].years == n * years
        for q, f in enumerate(("sum_lole", "sum_eue", "sum_lolf")):
            assert getattr(acc[j], f) == pytest.approx(yr[j][:, q].sum(), rel=1e-12), f
            assert getattr(acc[j], f + "2") == pytest.approx((yr[j][:, q] ** 2).sum(), rel=1e-12), f


@pytest.mark.gpu
@pytest.mark.parametrize("start", [M.ALL_UP, M.STATIONARY])
def test_whole_year_windows_are_the_sweeps_withheld_fleet_bitwise(engine, start):
    """Consequence 2 on fleet100 / 513 hours: units 3, 40, 70, 99 on maintenance the whole year == the sweep's fleet 1 with them withheld,
    at scale 1.07 and shift 33.25, alone and as one of three schedules."""
    _load(engine, *_fleet("513"))
    _, ref = _sweep_level(engine, 5, 2, 16, 5, start, 1.07, 33.25, 1, WH)
    _, all_units = _sweep_level(engine, 5, 2, 16, 5, start, 1.07, 33.25, 0)
    assert ref[:, 0].sum() > all_units[:, 0].sum() > 0
    whole = [(k, 0, 513) for k in WH]
    for sched, j in (([whole], 0), ([[], S513[1], whole], 2)):
        _, yr, _ = _run(engine, sched, 5, 2, 16, 5, start, 1.07, 33.25)
        assert yr[j].tobytes() == ref.tobytes(), len(sched)


@pytest.mark.gpu
@pytest.mark.parametrize("start", [M.ALL_UP, M.STATIONARY])
@pytest.mark.parametrize("fleet,schedules,n,years,shift", [("small", S168, 16, 7, 0.0), ("513", S513, 6, 3, 300.0)])
def test_schedules_equal_the_host_model(engine, fleet, schedules, n, years, shift, start):
    """Windows with their edges on the group, LDS-window and year boundaries: integers exact, EUE to rtol / atol 1e-9.  The 513-hour curve is
    raised by 300 MW, so that about half of all hours are loss hours and a window that is off by one hour changes the records."""
    cap, mttf, mttr, load = _fleet(fleet)
    _load(engine, cap, mttf, mttr, load)
    _, yr, _ = _run(engine, schedules, 5, 1, n, years, start, 1.0, shift)
    L, E, F = MM.maint_model(5, range(1, 1 + n), cap, mttf, mttr, load, years, start, schedules, 1.0, shift)
    assert L[0].sum() > 0 and all(L[j].sum() > L[0].sum() for j in range(1, len(schedules))) and F[1].sum() > n
    assert len({L[j].tobytes() + E[j].tobytes() for j in range(len(schedules))}) == len(schedules)
    np.testing.assert_array_equal(yr[:, :, 0], L)
    np.testing.assert_array_equal(yr[:, :, 2], F)
    np.testing.assert_allclose(yr[:, :, 1], E, rtol=1e-9, atol=1e-9)


@pytest.mark.gpu
def test_schedules_do_not_depend_on_each_other(engine):
    """Consequence 3: 8 schedules == 8 one-schedule calls; 2, 3 and 5 of them (kernels wider than the count) give the same records; a
    permutation permutes the records; one schedule at different positions beside different neighbours is bitwise equal."""
    _load(engine, *_fleet("513"))
    args = (5, 1, 16, 5, M.STATIONARY)
    _, all8, _ = _run(engine, S513, *args, 1.0, 300.0)
    assert len({all8[j].tobytes() for j in range(8)}) == 8 and all8[0][:, 0].sum() > 0
    for j in range(8):
        _, one, _ = _run(engine, [S513[j]], *args, 1.0, 300.0)
        assert one[0].tobytes() == all8[j].tobytes(), j
    for ns in (2, 3, 5):
        _, part, _ = _run(engine, S513[:ns], *args, 1.0, 300.0)
        assert part.tobytes() == all8[:ns].tobytes(), ns
    perm = np.random.default_rng(7).permutation(8)
    _, p8, _ = _run(engine, [S513[k] for k in perm], *args, 1.0, 300.0)
    assert p8.tobytes() == all8[perm].tobytes()
    _, rep, _ = _run(engine, [S513[3], S513[6], S513[3], S513[0], S513[3]], *args, 1.0, 300.0)
    assert rep[0].tobytes() == rep[2].tobytes() == rep[4].tobytes() == all8[3].tobytes() and rep[1].tobytes() == all8[6].tobytes()


@pytest.mark.gpu
def test_split_chunk_and_repeat_invariance(engine):
    """Consequence 3 over chain ranges: a range split into two calls, and a call that goes in several launches (8 schedules x 2^18 years
    per chain of a two-hour year: two chains to a launch, three chains to the call), equal the one call; a repeated call is bitwise
    identical, with and without the year records."""
    _load(engine, *_rts24())
    sched = [[], [(21, 1000, 700), (22, 8000, 1500)], [(12, 0, 8736)]]
    N, a, Y = 1000, 337, 2
    _maint_load(engine, sched)
    acc, yr, _ = _maint(engine, 7, 0, N, Y, M.STATIONARY, 3, 1.0, 50.0)
    acc1, yr1, _ = _maint(engine, 7, 0, a, Y, M.STATIONARY, 3, 1.0, 50.0)
    acc2, yr2, _ = _maint(engine, 7, a, N - a, Y, M.STATIONARY, 3, 1.0, 50.0)
    assert yr[0][:, 0].sum() > 0 and np.array_equal(yr, np.concatenate([yr1, yr2], axis=1))
    for j in range(3):
        assert acc[j].years == acc1[j].years + acc2[j].years == N * Y
        for f in ACC_FIELDS[1:]:
            assert getattr(acc[j], f) == pytest.approx(getattr(acc1[j], f) + getattr(acc2[j], f), rel=1e-12), f
    acc_r, yr_r, _ = _maint(engine, 7, 0, N, Y, M.STATIONARY, 3, 1.0, 50.0)
    acc_n, _, _ = _maint(engine, 7, 0, N, Y, M.STATIONARY, 3, 1.0, 50.0, want_years=False)
    assert yr.tobytes() == yr_r.tobytes()
    assert [_acc_tuple(x) for x in acc] == [_acc_tuple(x) for x in acc_r] == [_acc_tuple(x) for x in acc_n]
    # several launches: three units, a year of two hours
    _load(engine, np.array([30.0, 20.0, 10.0]), np.array([30.0, 25.0, 20.0]), np.array([10.0, 8.0, 6.0]), np.array([35.0, 45.0]))
    s8 = [[], [(0, 1, 1)], [(1, 1, 2)], [(2, 0, 1)], [(0, 0, 2)], [(1, 0, 1), (2, 1, 1)], [(2, 1, 2)], [(0, 1, 2), (1, 1, 1)]]
    Y = 1 << 18
    _maint_load(engine, s8)
    acc, yr, _ = _maint(engine, 3, 10, 3, Y, M.ALL_UP, 8)
    acc1, yr1, _ = _maint(engine, 3, 10, 1, Y, M.ALL_UP, 8)
    acc2, yr2, _ = _maint(engine, 3, 11, 2, Y, M.ALL_UP, 8)
    assert np.array_equal(yr[:, :Y], yr1) and np.array_equal(yr[:, Y:], yr2)
    assert len({yr[j].tobytes() for j in range(8)}) == 8 and yr[0][:, 0].sum() > 0
    for j in range(8):
        assert acc[j].years == 3 * Y
        for q, f in enumerate(("sum_lole", "sum_eue", "sum_lolf")):
            assert getattr(acc[j], f) == pytest.approx(yr[j][:, q].sum(), rel=1e-12), f
            assert getattr(acc[j], f) == pytest.approx(getattr(acc1[j], f) + getattr(acc2[j], f), rel=1e-12), f


@pytest.mark.gpu
def test_nested_schedules_are_ordered_exactly(engine):
    """Consequence 4: A contains B contains none in every hour -> every year's loss hours and EUE under A >= under B >= without."""
    _load(engine, *_fleet("513"))
    B = [(3, 30, 200), (70, 400, 150)]
    A = B + [(3, 200, 100), (99, 0, 513), (70, 380, 40), (12, 100, 300)]
    for start in (M.ALL_UP, M.STATIONARY):
        _, yr, _ = _run(engine, [A, B, []], 9, 0, 32, 4, start, 1.0, 10.0)
        for q in (0, 1):
            assert np.all(yr[0][:, q] >= yr[1][:, q]) and np.all(yr[1][:, q] >= yr[2][:, q])
        assert yr[0][:, 0].sum() > yr[1][:, 0].sum() > yr[2][:, 0].sum() > 0


@pytest.mark.gpu
def test_chain_counts(engine):
    """Seven chains (a workgroup with one idle wave), one chain, and no chain at all."""
    _load(engine, *_fleet("small"))
    _maint_load(engine, S168)
    _, yr8, _ = _maint(engine, 5, 3, 8, 4, M.STATIONARY, 4)
    acc7, yr7, _ = _maint(engine, 5, 3, 7, 4, M.STATIONARY, 4)
    acc1, yr1, _ = _maint(engine, 5, 3, 1, 4, M.STATIONARY, 4)
    assert yr8[1][:, 0].sum() > 0 and yr7.tobytes() == np.ascontiguousarray(yr8[:, :28]).tobytes() and yr1.tobytes() == np.ascontiguousarray(yr8[:, :4]).tobytes()
    assert all(acc7[j].years == 28 and acc1[j].years == 4 for j in range(4))
    acc0 = (_abi.Hl1SeqAcc * 4)()
    for a in acc0:
        a.years, a.sum_eue = -7, 3.5
    assert engine.L.relmc_hl1_maint_seq(engine._h, 5, 3, 0, 4, M.STATIONARY, 1.0, 0.0, acc0, None) == 0
    assert all(_acc_tuple(a) == (0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0) for a in acc0)


@pytest.mark.gpu
def test_error_codes(engine):
    L = engine.L
    h = C.c_void_p()
    assert L.relmc_ctx_create(0, C.byref(h)) == 0
    try:
        err = lambda: L.relmc_last_error(h).decode()
        ok = [[(1, 10, 20)], []]
        run = lambda n=4, years=2, start=0, scale=1.0, shift=0.0, ns=2: _maint(engine, 1, 0, n, years, start, ns, scale, shift, h=h)
        # RELMC_ERR_NO_CASE before either load call
        assert _maint_load(engine, ok, h=h) == -5 and "relmc_hl1_seq_load" in err()
        assert run()[2] == -5 and "relmc_hl1_seq_load" in err()
        assert _load(engine, *_fleet("small"), h=h) == 0
        assert run()[2] == -5 and "relmc_hl1_maint_load" in err()
        assert _maint_load(engine, ok, h=h) == 0
        good = run()
        assert good[2] == 0 and good[0][0].years == good[0][1].years == 8 and good[0][0].sum_lole > good[0][1].sum_lole > 0
        # relmc_hl1_maint_load's refusals: each names the window and the field, and the previous table still answers
        arr, n = _windows(ok)
        assert L.relmc_hl1_maint_load(None, 2, n, arr) == -1
        assert L.relmc_hl1_maint_load(h, 0, 0, None) == -1 and "n_schedules 0" in err()
        assert L.relmc_hl1_maint_load(h, 9, 0, None) == -1 and "n_schedules 9" in err()
        assert L.relmc_hl1_maint_load(h, 2, -1, arr) == -1 and "n_windows" in err()
        assert L.relmc_hl1_maint_load(h, 2, 1, None) == -1 and "without windows" in err()
        for bad, words in (((2, 0, 0, 1), ("window 1", "schedule 2")), ((-1, 0, 0, 1), ("window 1", "schedule -1")), ((0, 6, 0, 1), ("window 1", "unit 6")),
                           ((0, -1, 0, 1), ("window 1", "unit -1")), ((1, 0, 168, 1), ("window 1", "start_hour 168")), ((1, 0, -1, 1), ("window 1", "start_hour -1")),
                           ((1, 0, 0, 0), ("window 1", "hours 0")), ((1, 0, 0, 169), ("window 1", "hours 169"))):
            two = (_abi.Hl1MaintWindow * 2)(_abi.Hl1MaintWindow(0, 1, 10, 20), _abi.Hl1MaintWindow(*bad))
            assert L.relmc_hl1_maint_load(h, 2, 2, two) == -1 and all(w in err() for w in words), (bad, err())
        again = run()
        assert again[2] == 0 and again[1].tobytes() == good[1].tobytes()
        # relmc_hl1_maint_seq's refusals change nothing
        acc2 = (_abi.Hl1SeqAcc * 2)()
        for a in acc2:
            a.years, a.sum_lole = -7, 3.5
        yr = np.full((2, 8, 3), -7.0)
        for kw in (dict(scale=np.nan), dict(scale=np.inf), dict(shift=-np.inf), dict(start=2), dict(start=-1), dict(years=0), dict(n=-1)):
            a = dict(n=4, years=2, start=0, scale=1.0, shift=0.0)
            a.update(kw)
            assert L.relmc_hl1_maint_seq(h, 1, 0, a["n"], a["years"], a["start"], a["scale"], a["shift"], acc2, yr.ctypes.data_as(YP)) == -1, kw
            assert ("scale / shift" in err()) == ("scale" in kw or "shift" in kw)
        assert all((a.years, a.sum_lole) == (-7, 3.5) for a in acc2) and np.all(yr == -7.0)
        assert L.relmc_hl1_maint_seq(h, 1, 0, 4, 2, 0, 1.0, 0.0, None, None) == -1
        assert L.relmc_hl1_maint_seq(None, 1, 0, 4, 2, 0, 1.0, 0.0, acc2, None) == -1
        # another model: the run call is refused until the schedules are loaded again
        cap, mttf, mttr, load = _fleet("small")
        assert _load(engine, cap, mttf, mttr, load[:100], h=h) == 0
        assert run()[2] == -1 and "nhours" in err() and "168" in err() and "100" in err()
        assert _load(engine, cap[:5], mttf[:5], mttr[:5], load, h=h) == 0
        assert run()[2] == -1 and "ngen" in err()
        assert _maint_load(engine, ok, h=h) == 0 and run()[2] == 0
        assert _load(engine, cap, mttf, mttr, load, h=h) == 0 and _maint_load(engine, ok, h=h) == 0
        assert run()[1].tobytes() == good[1].tobytes()
    finally:
        L.relmc_ctx_destroy(h)


@pytest.fixture(scope="module")
def small_maintenance(engine):
    """The six-unit fleet, 20 000 one-year stationary chains, its 60 MW unit on maintenance for 48 hours mid-year beside no maintenance."""
    cap, mttf, mttr, load = M.small_fleet()
    gens = [hl1.Generator(i + 1, float(cap[i]), float(mttf[i]), float(mttr[i])) for i in range(cap.size)]
    sched = [[hm.MaintenanceWindow(0, 60, 48)], []]
    res = hm.run_sequential_maintenance(gens, hl1.LoadModel(load), sched, 20000, chains=20000, start="stationary", seed=21, engine=engine)
    return res, hm.run_analytical_maintenance(gens, hl1.LoadModel(load), sched)


@pytest.mark.gpu
def test_small_fleet_against_the_exact_answers(small_maintenance):
    """LOLE and EUE within 4.5 of their own standard errors of run_analytical_maintenance; LOLE strictly above the no-maintenance
    schedule's in the same call."""
    res, exact = small_maintenance
    print(hm.maintenance_report(res, exact))
    assert res.year_lole.shape == (2, 20000) and np.all(res.lole_se > 0)
    assert np.all(np.abs(res.lole_hours_yr - exact.lole_hours_yr) < 4.5 * res.lole_se), (res.lole_hours_yr, exact.lole_hours_yr, res.lole_se)
    assert np.all(np.abs(res.eue_mwh_yr - exact.eue_mwh_yr) < 4.5 * res.eue_se), (res.eue_mwh_yr, exact.eue_mwh_yr, res.eue_se)
    assert res.lole_hours_yr[0] > res.lole_hours_yr[1]
    np.testing.assert_allclose(res.lole_hours_yr, res.year_lole.mean(1), rtol=1e-12)


@pytest.mark.gpu
def test_paired_comparison_beats_the_unpaired_one(small_maintenance):
    res, _ = small_maintenance
    c = hm.compare_schedules(res, base=1)
    assert c.d_lole[0] == pytest.approx(res.lole_hours_yr[0] - res.lole_hours_yr[1], rel=1e-9) and c.d_lole[0] > 0 and c.d_eue[0] > 0
    for paired, unpaired in ((c.d_lole_se, c.d_lole_se_unpaired), (c.d_eue_se, c.d_eue_se_unpaired), (c.d_lolf_se, c.d_lolf_se_unpaired)):
        assert 0 < paired[0] < unpaired[0] and paired[1] == 0.0
    assert np.all(res.year_lole[0] >= res.year_lole[1]) and np.all(res.year_eue[0] >= res.year_eue[1])


@pytest.mark.gpu
def test_python_empty_schedule_is_run_sequential_mc(engine):
    gens, load = hl1.rts24_generators(), hl1.rts24_load()
    ref = hl1.run_sequential_mc(gens, load, 30, seed=2, engine=engine)
    res = hm.run_sequential_maintenance(gens, load, [[], hm.levelised_schedule(gens, load, [2] * 32)], 30, seed=2, engine=engine)
    r = res.result(0)
    for f in ("year_lole", "year_eue", "year_lolf", "convergence_history"):
        assert getattr(r, f).tobytes() == getattr(ref, f).tobytes(), f
    assert (r.lole_hours_yr, r.eue_mwh_yr, r.lolf_occ_yr) == (ref.lole_hours_yr, ref.eue_mwh_yr, ref.lolf_occ_yr)
    assert res.lole_hours_yr[1] > res.lole_hours_yr[0] and "Schedule" in hl1.compare_results([res.result(0), res.result(1)])
