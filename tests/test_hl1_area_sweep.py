"""Sweep of the HL1 multi-area chronology on the GPU (relmc_hl1_area_sweep): every level bitwise against relmc_hl1_area on the model it is
equivalent to, the identity and isolated levels, level independence, the host model (tests/tools/hl1_area_sweep_model.py), exact
monotonicity of the system row under MAX_FLOW, split / repeat invariance, the error codes, the neighbours left alone, and the three
searches against the exact stationary answer."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from powersystemsreliabilityassessment_amd import _abi, hl1, hl1_areas

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("hl1_area_sweep_model", os.path.join(ROOT, "tests", "tools", "hl1_area_sweep_model.py"))
SM = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(SM)
TM, AM = SM.TM, SM.AM

dp, ip = _abi.c_double_p, _abi.c_int32_p
FLOWS = [SM.REFERENCE, SM.MAX_FLOW]
ISO, INT = SM.ISOLATED, SM.INTERCONNECTED


# ---- the C ABI, raw ---------------------------------------------------------------------------------------------------------------
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


def _outages(eng, kf, kr):
    if kf is None:
        rc = eng.L.relmc_hl1_area_tie_outages(eng._h, 0, None, None)
    else:
        kf, kr = np.ascontiguousarray(kf, dtype=np.float64), np.ascontiguousarray(kr, dtype=np.float64)
        rc = eng.L.relmc_hl1_area_tie_outages(eng._h, kf.size, kf.ctypes.data_as(dp), kr.ctypes.data_as(dp))
    eng._check(rc, "relmc_hl1_area_tie_outages")
    eng._hl1_area_loaded = None


def _run(eng, rows, seed, first, n, years, start, policy, flow):
    acc = (_abi.Hl1SeqAcc * rows)()
    yr = np.zeros((n * years, rows, 3))
    eng._check(eng.L.relmc_hl1_area(eng._h, seed, first, n, years, start, policy, flow, acc, yr.ctypes.data_as(C.POINTER(_abi.Hl1SeqYear))),
               "relmc_hl1_area")
    return acc, yr


def _levels(levels, n):
    """ctypes array of relmc_hl1_area_level from (scale, shift, tie_scale, fleet) tuples; the entries at or above n are NaN: not read."""
    arr = (_abi.Hl1AreaLevel * len(levels))()
    for j, (scale, shift, ts, fleet) in enumerate(levels):
        arr[j].load_scale[:] = np.broadcast_to(np.asarray(scale, float), (n,)).tolist() + [float("nan")] * (8 - n)
        arr[j].load_shift[:] = np.broadcast_to(np.asarray(shift, float), (n,)).tolist() + [float("nan")] * (8 - n)
        arr[j].tie_scale, arr[j].fleet, arr[j].reserved = float(ts), int(fleet), 0
    return arr


def _mask(withheld):
    if withheld is None:
        return None
    m = (C.c_uint32 * 4)()
    for k in withheld:
        m[k >> 5] |= 1 << (k & 31)
    return m


def _sweep_rc(L, h, rows, seed, first, n, years, start, flow, levels, withheld=None, tie_scaled=None, acc=True, nl=None):
    arr = _levels(levels, rows - 1) if levels is not None else None
    nl = (len(levels) if levels is not None else 1) if nl is None else nl
    a = (_abi.Hl1SeqAcc * (max(nl, 1) * rows))()
    yr = np.zeros((max(nl, 1), max(n, 0) * max(years, 0), rows, 3))
    ts = None if tie_scaled is None else np.ascontiguousarray(tie_scaled, dtype=np.uint8)
    rc = L.relmc_hl1_area_sweep(h, seed, first, n, years, start, flow, nl, arr, _mask(withheld),
                                None if ts is None else ts.ctypes.data_as(_abi.c_uint8_p), a if acc else None,
                                yr.ctypes.data_as(C.POINTER(_abi.Hl1SeqYear)))
    return rc, a, yr


def _sweep(eng, rows, seed, first, n, years, start, flow, levels, withheld=None, tie_scaled=None):
    rc, acc, yr = _sweep_rc(eng.L, eng._h, rows, seed, first, n, years, start, flow, levels, withheld, tie_scaled)
    eng._check(rc, "relmc_hl1_area_sweep")
    return acc, yr


def _acc_tuple(acc):
    return [tuple(getattr(x, f) for f, _ in _abi.Hl1SeqAcc._fields_) for x in acc]


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
def _fleet5():
    """test_hl1_tie.py's 5-area fleet: 100 units in areas of 20 (both cursor slots), a 1000-hour year (windows straddle years), 7 ties of
    which ties 1 and 6 are parallel (areas 1-2), all failing."""
    cap, mttf, mttr, load = AM.SEQ.fleet100()
    h = np.arange(load.size)
    share = np.array([cap[20 * a:20 * a + 20] @ (mttf / (mttf + mttr))[20 * a:20 * a + 20] for a in range(5)])
    loads = np.stack([share[a] * (0.9 + 0.06 * np.sin(2 * np.pi * (h - 5 * a) / 24.0) + 0.03 * np.sin(2 * np.pi * h / (300.0 + 90 * a)))
                      for a in range(5)])
    ties = [(0, 1, 40.0), (1, 2, 25.5), (2, 3, 60.0), (3, 4, 15.25), (4, 0, 30.0), (0, 2, 10.0), (1, 2, 5.0)]
    kf = np.array([400.0, 650.0, 300.0, 520.0, 480.0, 350.0, 275.0])
    kr = np.array([30.0, 45.0, 25.0, 60.0, 35.0, 40.0, 20.0])
    return [20] * 5, cap, mttf, mttr, loads, ties, kf, kr


WITHHELD5 = [7, 85]                                  # a unit below 64 and one at or above 64 (the second cursor slot)
SCALED5 = [1, 1, 1, 1, 1, 1, 0]                      # tie 6, the parallel of tie 1, keeps its capacity
LEVELS5 = [
    (1.0, 0.0, 1.0, 0),
    ([1.02, 0.97, 1.0, 1.05, 0.99], [3.5, -2.25, 0.0, 10.0, -7.125], 0.5, 0),
    (1.0, 0.0, 0.0, 0),
    (1.0, 12.0, 2.5, 0),
    (1.0, 0.0, 1.0, 1),
    (1.03, 0.0, 0.5, 1),
    (1.04, 0.0, 1.0, 0),
    (1.0, [20.0, 0.0, 0.0, 0.0, -5.0], 2.5, 0),
]


def _arrays(sysm):
    g = [x for a in sysm.areas for x in a.generators]
    return ([len(a.generators) for a in sysm.areas], np.array([x.capacity for x in g]), np.array([x.mttf for x in g]),
            np.array([x.mttr for x in g]), np.stack([np.asarray(a.hourly_load, dtype=np.float64) for a in sysm.areas]),
            [(t.from_area - 1, t.to_area - 1, float(t.capacity)) for t in sysm.tie_lines])


def _rts96_raised():
    units, cap, mttf, mttr, loads, ties = _arrays(hl1_areas.rts96_system(tie_outages=True))
    return units, cap, mttf, mttr, loads * np.array([[1.18], [1.0], [1.22]]), ties


# ---- 1. bitwise equivalence to the transformed model --------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("outages", [False, True])
@pytest.mark.parametrize("flow", FLOWS)
def test_every_level_is_bitwise_the_transformed_model(engine, flow, outages):
    units, cap, mttf, mttr, loads, ties, kf, kr = _fleet5()
    shapes = [(3, 2, 1, 20), (9, 0, 48, 2)]                                   # (seed, first chain, chains, years)
    cases = [(sh, st) for sh in shapes for st in (SM.ALL_UP, SM.STATIONARY)]
    _load(engine, units, cap, mttf, mttr, loads, ties)
    if outages:
        _outages(engine, kf, kr)
    got = {c: _sweep(engine, 6, c[0][0], c[0][1], c[0][2], c[0][3], c[1], flow, LEVELS5, WITHHELD5, SCALED5)[1] for c in cases}
    try:
        for j, level in enumerate(LEVELS5):
            c_j, ld_j, ties_j = SM.transform(cap, loads, ties, level, WITHHELD5, SCALED5)
            _load(engine, units, c_j, mttf, mttr, ld_j, ties_j)
            if outages:
                _outages(engine, kf, kr)
            for (seed, first, n, years), start in cases:
                _, want = _run(engine, 6, seed, first, n, years, start, INT, flow)
                assert got[((seed, first, n, years), start)][j].tobytes() == want.tobytes(), (j, n, years, start)
    finally:
        _load(engine, units, cap, mttf, mttr, loads, ties)                    # the original model again
    for c, yr in got.items():
        assert (yr[:, :, 5, 0].sum(1) >= 1).all(), c                          # every level's system row has a loss hour
        distinct = {yr[j].tobytes() for j in range(len(LEVELS5))}
        assert len(distinct) >= 3, c


@pytest.mark.gpu
def test_eight_areas_and_eight_levels(engine):
    """The largest LDS footprint (8 areas x 8 levels, beyond 64 KB per workgroup): identity = INTERCONNECTED, tie scale 0 = ISOLATED, and
    a shifted level against its transformed model."""
    rng = np.random.default_rng(5)
    units = [2] * 8
    cap = rng.integers(20, 60, 16).astype(float)
    mttf, mttr = rng.uniform(200.0, 400.0, 16), rng.uniform(20.0, 60.0, 16)
    h = np.arange(700)
    loads = np.stack([0.8 * cap[2 * a:2 * a + 2].sum() * (0.85 + 0.1 * np.sin(2 * np.pi * (h + 3 * a) / 24.0)) for a in range(8)])
    ties = [(a, (a + 1) % 8, 10.0 + a) for a in range(8)] + [(0, 4, 7.5)]
    levels = [(1.0, 0.0, 1.0, 0), (1.0, 0.0, 0.0, 0), (1.05, -2.0, 1.5, 0)] + [(1.0, float(k), 1.0, 0) for k in range(1, 6)]
    for flow in FLOWS:
        _load(engine, units, cap, mttf, mttr, loads, ties)
        _, yr = _sweep(engine, 9, 2, 0, 8, 3, SM.STATIONARY, flow, levels)
        assert yr[0].tobytes() == _run(engine, 9, 2, 0, 8, 3, SM.STATIONARY, INT, flow)[1].tobytes()
        assert yr[1].tobytes() == _run(engine, 9, 2, 0, 8, 3, SM.STATIONARY, ISO, flow)[1].tobytes()
        c_j, ld_j, ties_j = SM.transform(cap, loads, ties, levels[2])
        _load(engine, units, c_j, mttf, mttr, ld_j, ties_j)
        assert yr[2].tobytes() == _run(engine, 9, 2, 0, 8, 3, SM.STATIONARY, INT, flow)[1].tobytes()
        assert yr[0, :, 8, 0].sum() > 0 and yr[0].tobytes() != yr[1].tobytes()


# ---- 2. identity and isolated levels -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("system", ["demo", "rts96"])
def test_identity_and_isolated_levels(engine, system):
    if system == "demo":
        units, cap, mttf, mttr, loads, ties = _arrays(hl1_areas.demo_system())
        n, years = 64, 2
    else:
        units, cap, mttf, mttr, loads, ties = _rts96_raised()
        n, years = 16, 2
    rows = len(units) + 1
    _load(engine, units, cap, mttf, mttr, loads, ties)
    for flow in FLOWS:
        for start in (SM.ALL_UP, SM.STATIONARY):
            acc, yr = _sweep(engine, rows, 5, 3, n, years, start, flow, [(1.0, 0.0, 1.0, 0), (1.0, 0.0, 0.0, 0)])
            acc_i, inter = _run(engine, rows, 5, 3, n, years, start, INT, flow)
            acc_0, iso = _run(engine, rows, 5, 3, n, years, start, ISO, flow)
            assert yr[0].tobytes() == inter.tobytes() and yr[1].tobytes() == iso.tobytes(), (flow, start)
            assert inter.tobytes() != iso.tobytes() and iso[:, -1, 0].sum() > 0
            assert _acc_tuple(acc[:rows]) == _acc_tuple(acc_i) and _acc_tuple(acc[rows:]) == _acc_tuple(acc_0)
            for j in range(2):
                for r in range(rows):
                    a = acc[j * rows + r]
                    assert a.years == n * years
                    for q, f in enumerate(("sum_lole", "sum_eue", "sum_lolf")):
                        assert getattr(a, f) == pytest.approx(yr[j, :, r, q].sum(), rel=1e-12)
                        assert getattr(a, f + "2") == pytest.approx((yr[j, :, r, q] ** 2).sum(), rel=1e-12)


# ---- 3. level independence -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_levels_records_do_not_depend_on_the_other_levels(engine):
    units, cap, mttf, mttr, loads, ties, kf, kr = _fleet5()
    _load(engine, units, cap, mttf, mttr, loads, ties)
    _outages(engine, kf, kr)
    args = (6, 4, 1, 12, 3, SM.STATIONARY, SM.MAX_FLOW)
    _, full = _sweep(engine, *args, LEVELS5, WITHHELD5, SCALED5)
    for pick in ([5], [7, 2], [4, 0, 6], [3, 1, 5, 2, 7], [7, 6, 5, 4, 3, 2, 1, 0]):       # 1, 2, 3, 5 and 8 levels, in other orders
        _, part = _sweep(engine, *args, [LEVELS5[j] for j in pick], WITHHELD5, SCALED5)
        for q, j in enumerate(pick):
            assert part[q].tobytes() == full[j].tobytes(), (pick, j)
    _outages(engine, None, None)


# ---- 4. the host model ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("flow,start", [(SM.REFERENCE, SM.STATIONARY), (SM.MAX_FLOW, SM.ALL_UP)])
def test_device_equals_host_model(engine, flow, start):
    """The demo system with its tie at 950 h / 50 h, 16 chains x 2 years, 8 levels: integers exact, EUE to 1e-9."""
    units, cap, mttf, mttr, loads, ties = _arrays(hl1_areas.demo_system())
    levels = [(1.0, 0.0, 1.0, 0), (1.0, 0.0, 0.0, 0), (1.0, [0.0, -150.0], 0.25, 0), ([1.1, 0.9], [25.0, 0.5], 2.0, 0), (1.0, 0.0, 1.0, 1),
              (0.95, 40.0, 0.5, 1), (1.0, [100.0, 0.0], 1.5, 0), (1.0, -200.0, 1.0, 0)]
    _load(engine, units, cap, mttf, mttr, loads, ties)
    _outages(engine, [950.0], [50.0])
    _, yr = _sweep(engine, 3, 11, 40, 16, 2, start, flow, levels, [2, 8])
    _outages(engine, None, None)
    model = SM.sweep_model(11, range(40, 56), units, cap, mttf, mttr, loads, ties, [950.0], [50.0], 2, start, flow, levels, [2, 8])
    np.testing.assert_array_equal(yr[..., 0], model[..., 0])
    np.testing.assert_array_equal(yr[..., 2], model[..., 2])
    np.testing.assert_allclose(yr[..., 1], model[..., 1], rtol=1e-9, atol=1e-9)
    assert (model[:, :, 2, 0].sum(1) > 1000).all()                                        # thousands of loss hours in every level


# ---- 5. monotonicity -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_system_row_is_monotone_in_tie_scale_and_shift_under_max_flow(engine):
    """Integer loads and capacities, tie scales k / 4 and integer shifts: every margin, capacity and flow is an exact multiple of 1/4 far
    above the 1e-4 thresholds, so the maximum flow's monotonicity holds year by year, exactly."""
    units, cap, mttf, mttr, loads, ties = _arrays(hl1_areas.demo_system())
    _load(engine, units, cap, mttf, mttr, np.round(loads), ties)
    scales = [0.0, 0.25, 0.5, 0.75, 1.0, 1.25, 1.5, 2.0]
    _, yr = _sweep(engine, 3, 8, 0, 256, 1, SM.STATIONARY, SM.MAX_FLOW, [(1.0, 0.0, s, 0) for s in scales])
    for q in (0, 1):
        d = np.diff(yr[:, :, 2, q], axis=0)
        assert (d <= 0).all() and d.sum(1).max() < 0, q                                   # nonincreasing, and every step of the scale helps
    shifts = [-120.0, -45.0, -1.0, 0.0, 2.0, 30.0, 77.0, 160.0]
    for a in (0, 1):
        _, yr = _sweep(engine, 3, 8, 0, 256, 1, SM.STATIONARY, SM.MAX_FLOW, [(1.0, [s if b == a else 0.0 for b in range(2)], 1.0, 0) for s in shifts])
        for q in (0, 1):
            d = np.diff(yr[:, :, 2, q], axis=0)
            assert (d >= 0).all() and d.sum(1).min() > 0, (a, q)


# ---- 6. invariance and isolation -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_split_and_repeat_invariance(engine):
    units, cap, mttf, mttr, loads, ties, kf, kr = _fleet5()
    _load(engine, units, cap, mttf, mttr, loads, ties)
    _outages(engine, kf, kr)
    N, a, Y = 300, 101, 2
    args = lambda first, n: (6, 7, first, n, Y, SM.STATIONARY, SM.MAX_FLOW, LEVELS5[:5], WITHHELD5, SCALED5)
    acc, yr = _sweep(engine, *args(0, N))
    acc1, yr1 = _sweep(engine, *args(0, a))
    acc2, yr2 = _sweep(engine, *args(a, N - a))
    _outages(engine, None, None)
    assert np.array_equal(yr, np.concatenate([yr1, yr2], axis=1))
    for s in range(5 * 6):
        assert acc[s].years == acc1[s].years + acc2[s].years == N * Y
        for f in ("sum_lole", "sum_eue", "sum_lolf", "sum_lole2", "sum_eue2", "sum_lolf2"):
            assert getattr(acc[s], f) == pytest.approx(getattr(acc1[s], f) + getattr(acc2[s], f), rel=1e-12), f
    _outages(engine, kf, kr)
    acc_r, yr_r = _sweep(engine, *args(0, N))
    _outages(engine, None, None)
    assert np.array_equal(yr, yr_r) and _acc_tuple(acc) == _acc_tuple(acc_r)


@pytest.mark.gpu
def test_long_chain_ranges_go_in_several_launches(engine):
    """24 record slices (8 levels x 3 rows) x 64 years: a launch holds 2730 chains at most, so 2800 chains take two.  The records of the
    chains on both sides of the cut equal those of short calls of their own, and acc the sums of the records."""
    units, cap, mttf, mttr, loads, ties = _arrays(hl1_areas.demo_system(hours=24))
    _load(engine, units, cap, mttf, mttr, loads, ties)
    levels = [(1.0, 10.0 * k, 0.25 * k, 0) for k in range(8)]
    acc, yr = _sweep(engine, 3, 6, 0, 2800, 64, SM.STATIONARY, SM.MAX_FLOW, levels)
    _, cut = _sweep(engine, 3, 6, 2700, 100, 64, SM.STATIONARY, SM.MAX_FLOW, levels)
    assert np.array_equal(yr[:, 2700 * 64:], cut) and yr[:, 2730 * 64:, 2, 0].sum() > 0
    # a 24-hour year: every 64-step group spans years.  Level 0 (tie scale 0) is ISOLATED, level 4 its transformed model.
    assert cut[0].tobytes() == _run(engine, 3, 6, 2700, 100, 64, SM.STATIONARY, ISO, SM.MAX_FLOW)[1].tobytes()
    c_j, ld_j, ties_j = SM.transform(cap, loads, ties, levels[4])
    _load(engine, units, c_j, mttf, mttr, ld_j, ties_j)
    assert cut[4].tobytes() == _run(engine, 3, 6, 2700, 100, 64, SM.STATIONARY, INT, SM.MAX_FLOW)[1].tobytes()
    for s in range(24):
        j, r = divmod(s, 3)
        assert acc[s].years == 2800 * 64
        for q, f in enumerate(("sum_lole", "sum_eue", "sum_lolf")):
            assert getattr(acc[s], f) == pytest.approx(yr[j, :, r, q].sum(), rel=1e-12)


@pytest.mark.gpu
def test_error_codes(engine):
    L = engine.L
    h = C.c_void_p()
    assert L.relmc_ctx_create(0, C.byref(h)) == 0
    try:
        ok = [(1.0, 0.0, 1.0, 0), (1.0, 5.0, 0.5, 1)]
        sweep = lambda levels=ok, withheld=(7, 85), **kw: _sweep_rc(L, h, 6, 5, 0, kw.pop("n", 8), kw.pop("years", 2), kw.pop("start", 1),
                                                                   kw.pop("flow", 1), levels, withheld, **kw)
        assert sweep()[0] == -5                                                       # RELMC_ERR_NO_CASE before a load
        assert _sweep_rc(L, None, 6, 5, 0, 8, 2, 1, 1, ok, (7, 85))[0] == -1
        units, cap, mttf, mttr, loads, ties, kf, kr = _fleet5()
        u = np.ascontiguousarray(units, dtype=np.int32)
        arrs = [np.ascontiguousarray(x, dtype=np.float64) for x in (cap[:90], mttf[:90], mttr[:90], loads)]
        u[4] = 10                                                                     # 90 units: the bits 90 .. 127 are out of range
        tf = np.ascontiguousarray([t[0] for t in ties], dtype=np.int32)
        tt = np.ascontiguousarray([t[1] for t in ties], dtype=np.int32)
        tc = np.ascontiguousarray([t[2] for t in ties], dtype=np.float64)
        assert L.relmc_hl1_area_load(h, 5, u.ctypes.data_as(ip), *[a.ctypes.data_as(dp) for a in arrs[:3]], 1000, arrs[3].ctypes.data_as(dp),
                                     7, tf.ctypes.data_as(ip), tt.ctypes.data_as(ip), tc.ctypes.data_as(dp)) == 0

        def area_run():
            acc = (_abi.Hl1SeqAcc * 6)()
            yr = np.zeros((16, 6, 3))
            assert L.relmc_hl1_area(h, 5, 0, 8, 2, 1, 1, 1, acc, yr.ctypes.data_as(C.POINTER(_abi.Hl1SeqYear))) == 0
            return yr

        base = area_run()
        rc, acc0, ref = sweep()
        assert rc == 0 and ref[0].tobytes() == base.tobytes()
        lv = lambda **kw: [ok[0], tuple(kw.get(k, d) for k, d in zip(("scale", "shift", "ts", "fleet"), ok[1]))]
        bad = [
            (dict(levels=None), b"bad arguments"), (dict(acc=False), b"bad arguments"), (dict(n=-1), b"bad arguments"),
            (dict(years=0), b"bad arguments"), (dict(start=2), b"bad arguments"), (dict(flow=2), b"bad arguments"),
            (dict(nl=0), b"n_levels 0"), (dict(levels=[ok[0]] * 9), b"n_levels 9"),
            (dict(levels=lv(scale=[1.0, 1.0, np.nan, 1.0, 1.0])), b"level 1: load scale / shift of area 2"),
            (dict(levels=lv(shift=[0.0, 0.0, 0.0, 0.0, np.inf])), b"level 1: load scale / shift of area 4"),
            (dict(levels=lv(ts=-0.5)), b"level 1: tie_scale"), (dict(levels=lv(ts=np.nan)), b"level 1: tie_scale"),
            (dict(levels=lv(ts=np.inf)), b"level 1: tie_scale"), (dict(levels=lv(ts=1e308)), b"level 1: scaled capacity of tie 0"),
            (dict(levels=lv(fleet=2)), b"level 1: fleet 2"), (dict(withheld=None), b"level 1: fleet 1 without"),
            (dict(withheld=(7, 90)), b"withheld bit 90"), (dict(withheld=(127,)), b"withheld bit 127"),
        ]
        for kw, msg in bad:
            assert sweep(**kw)[0] == -1, kw
            assert msg in L.relmc_last_error(h), (kw, L.relmc_last_error(h))
            rc, acc, yr = sweep()                                                     # a refused call changes nothing
            assert rc == 0 and yr.tobytes() == ref.tobytes() and _acc_tuple(acc) == _acc_tuple(acc0), kw
        arr = _levels(ok, 5)
        arr[1].reserved = 1
        a = (_abi.Hl1SeqAcc * 12)()
        assert L.relmc_hl1_area_sweep(h, 5, 0, 8, 2, 1, 1, 2, arr, _mask((7,)), None, a, None) == -1 and b"level 1: reserved" in L.relmc_last_error(h)
        # the entries at or above n_areas are not read (_levels fills them with NaN); n_chains = 0 zeroes the outputs
        rc, acc, yr = sweep(n=0)
        assert rc == 0 and all(x.years == 0 and x.sum_eue == 0.0 for x in acc)
        # years_host is optional; the loaded model is what it was
        a = (_abi.Hl1SeqAcc * 12)()
        assert L.relmc_hl1_area_sweep(h, 5, 0, 8, 2, 1, 1, 2, _levels(ok, 5), _mask((7, 85)), None, a, None) == 0
        assert _acc_tuple(a) == _acc_tuple(acc0)
        assert area_run().tobytes() == base.tobytes()
    finally:
        L.relmc_ctx_destroy(h)


@pytest.mark.gpu
def test_the_other_models_and_the_loaded_model_are_left_alone(engine):
    gens, load = hl1.rts24_generators(), hl1.rts24_load()
    before = hl1.run_non_sequential_mc(gens, load, 20000, seed=3, engine=engine)
    before_seq = hl1.run_sequential_mc(gens, load, 20, seed=3, engine=engine)
    before_sweep = hl1.run_load_sweep(gens, load, 20, [hl1.SweepLevel(), hl1.SweepLevel(1.0, 100.0)], seed=3, engine=engine)
    units, cap, mttf, mttr, loads, ties, kf, kr = _fleet5()
    _load(engine, units, cap, mttf, mttr, loads, ties)
    _outages(engine, kf, kr)
    area0 = {(p, f): _run(engine, 6, 1, 0, 32, 1, SM.STATIONARY, p, f)[1] for p in (ISO, INT) for f in FLOWS}
    _sweep(engine, 6, 1, 0, 32, 1, SM.STATIONARY, SM.MAX_FLOW, LEVELS5, WITHHELD5, SCALED5)
    for (p, f), want in area0.items():
        assert _run(engine, 6, 1, 0, 32, 1, SM.STATIONARY, p, f)[1].tobytes() == want.tobytes(), (p, f)
    _outages(engine, None, None)
    after = hl1.run_non_sequential_mc(gens, load, 20000, seed=3, engine=engine)
    after_seq = hl1.run_sequential_mc(gens, load, 20, seed=3, engine=engine)
    after_sweep = hl1.run_load_sweep(gens, load, 20, [hl1.SweepLevel(), hl1.SweepLevel(1.0, 100.0)], seed=3, engine=engine)
    assert (before.lole_hours_yr, before.eue_mwh_yr) == (after.lole_hours_yr, after.eue_mwh_yr)
    assert np.array_equal(before_seq.year_lole, after_seq.year_lole) and np.array_equal(before_seq.year_eue, after_seq.year_eue)
    assert np.array_equal(before_sweep.year_eue, after_sweep.year_eue) and np.array_equal(before_sweep.year_lolf, after_sweep.year_lolf)


# ---- 7. the Python surface and the searches ------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_python_surface(engine):
    d = hl1_areas.demo_system()
    sysm = hl1_areas.System(d.areas, [hl1_areas.TieLine(1, 2, 200.0, 950.0, 50.0)])
    levels = [hl1_areas.AreaSweepLevel(), hl1_areas.AreaSweepLevel(tie_scale=0.0), hl1_areas.AreaSweepLevel(load_shift=[0.0, -100.0], withheld=True),
              hl1_areas.AreaSweepLevel(load_scale=1.05, tie_scale=2.0)]
    kw = dict(seed=2, chains=64, start="stationary", engine=engine)
    sw = hl1_areas.run_area_sweep(sysm, 128, levels, withheld_units=[6], flow="max_flow", **kw)
    run = hl1_areas.run_fast_sequential_simulation
    assert sw.lole.shape == sw.eue_se.shape == (4, 3) and sw.year_indices.shape == (4, 128, 3, 3) and sw.scaled_ties == (0,)
    for j, lv in enumerate(levels):
        ref = run(hl1_areas.level_system(sysm, lv, withheld_units=[6]), hl1_areas.INTERCONNECTED, 128, flow="max_flow", **kw)
        assert sw.year_indices[j].tobytes() == ref.year_indices.tobytes(), j
        assert sw.lole[j, 2] == ref.system_lole and sw.eue[j, 1] == ref.results[1].eue and sw.lolf[j, 0] == ref.lolf[0]
    iso = run(sysm, hl1_areas.ISOLATED, 128, **kw)
    assert sw.year_indices[1].tobytes() == iso.year_indices.tobytes()
    np.testing.assert_allclose(sw.eue_se[0], sw.year_indices[0, :, :, 1].std(axis=0, ddof=1) / np.sqrt(128), rtol=1e-12)
    rep = hl1_areas.area_sweep_report(sw)
    assert "=== MULTI-AREA SWEEP (INTERCONNECTED, max_flow) ===" in rep and "| Area_Poor  |" in rep and "| SYSTEM     |" in rep
    assert "w/o: the fleet without units [6]" in rep


def _exact_root(f, target, lo, hi, tol=0.02):
    """x in [lo, hi] with f(x) = target for a continuous nondecreasing f: regula falsi with the Illinois rule, stopped on the bracket."""
    flo, fhi = f(lo) - target, f(hi) - target
    assert flo <= 0.0 <= fhi
    side = 0
    for _ in range(60):
        if hi - lo <= tol:
            break
        x = (lo * fhi - hi * flo) / (fhi - flo)
        if not lo < x < hi or min(x - lo, hi - x) < 0.25 * tol:                           # keep the bracket shrinking from both ends
            x = 0.5 * (lo + hi)
        fx = f(x) - target
        if fx <= 0.0:
            lo, flo = x, fx
            if side == -1:
                fhi *= 0.5
            side = -1
        else:
            hi, fhi = x, fx
            if side == 1:
                flo *= 0.5
            side = 1
    return 0.5 * (lo + hi)


@pytest.mark.gpu
def test_searches_against_the_exact_stationary_answer(engine):
    """Demo system, stationary start, MAX_FLOW, system row: interconnection_benefit and area_load_carrying_capability within 4 of their own
    reported standard errors of the root of hl1_area_model.joint_stationary on the shifted system (p ~ 6e-5 per check at a fixed seed)."""
    d = hl1_areas.demo_system()
    units, cap, mttf, mttr, loads, ties = _arrays(d)
    T = AM.topology(2, ties)
    area = 2

    def exact(x, policy, q):
        ld = loads.copy()
        ld[area - 1] = ld[area - 1] + x
        return AM.joint_stationary(units, cap.astype(int), mttf, mttr, ld, T, policy, SM.MAX_FLOW)[2, q]

    kw = dict(seed=12, chains=4096, start="stationary", flow="max_flow", engine=engine)
    for metric, q in (("lole", 0), ("eue", 1)):
        iso = exact(0.0, ISO, q)
        want = _exact_root(lambda x: exact(x, INT, q), iso, 0.0, 250.0)     # far finer than any standard error below
        res = hl1_areas.interconnection_benefit(d, area, 4096, metric=metric, row="system", **kw)
        print(f"benefit {metric}: {res.value:.3f} +- {res.std_error:.3f}, exact {want:.3f}, target {res.target:.2f} (exact {iso:.2f})")
        assert np.isfinite(res.std_error) and 0 < res.std_error < 20.0
        assert abs(res.value - want) < 4.0 * res.std_error, (metric, res.value, want, res.std_error)
        assert len(res.target_year) == 3 and all(np.array_equal(res.target_year[0], t) for t in res.target_year[1:])
        target = exact(50.0, INT, q)
        res = hl1_areas.area_load_carrying_capability(d, area, target, 4096, metric=metric, row="system", bracket=(-100.0, 300.0), **kw)
        print(f"carrying capability {metric}: {res.value:.3f} +- {res.std_error:.3f}, exact 50")
        want = 50.0                                                                   # by construction: the exact metric rises with the load
        assert abs(res.value - want) < 4.0 * res.std_error, (metric, res.value, want, res.std_error)
    res = hl1_areas.unit_elcc(d, [5], area, 4096, row="system", **kw)                 # one 200 MW unit of Area_Poor
    assert 0.0 < res.value < 200.0 and res.pair[0] <= res.value <= res.pair[1] and np.isfinite(res.std_error)
    with pytest.raises(ValueError):                                                   # the target lies outside the bracket
        hl1_areas.area_load_carrying_capability(d, area, 1.0, 256, row="system", bracket=(0.0, 10.0),
                                                **{**kw, "chains": 256})
