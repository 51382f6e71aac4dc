"""Energy storage on the HL1 sequential chronology on the GPU (relmc_hl1_seq_storage): storages without effect against relmc_hl1_seq and
relmc_hl1_seq_sweep bit for bit, the host model (tests/tools/hl1_storage_model.py) on shapes that carry state of charge and events across
windows and years, the invariants, a pattern worked out by hand, eight storages, split / repeat invariance, the error codes, and the
Python layer of hl1_storage.py."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from powersystemsreliabilityassessment_amd import _abi, hl1, hl1_storage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("hl1_storage_model", os.path.join(ROOT, "tests", "tools", "hl1_storage_model.py"))
SM = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(SM)
M = SM.SEQ

dp = _abi.c_double_p
ACC_FIELDS = [f for f, _ in _abi.Hl1StorageAcc._fields_]
# (charge_mw, discharge_mw, energy_mwh, eta_charge, eta_discharge, soc0_mwh); the first two sets are those of tests/test_hl1_storage_host.py
SMALL_STORAGES = [(20.0, 20.0, 60.0, 0.9, 0.95, 60.0), (10.0, 15.0, 30.0, 0.85, 1.0, 0.0)]
F513_STORAGES = [(30.0, 30.0, 90.0, 0.9, 0.9, 90.0), (15.0, 25.0, 40.0, 0.8, 1.0, 0.0), (5.0, 5.0, 1000.0, 1.0, 1.0, 500.0)]
DAY_STORAGES = [(25.0, 40.0, 120.0, 0.95, 0.9, 60.0), (8.0, 8.0, 16.0, 1.0, 0.75, 16.0)]
BATTERY = [(100.0, 100.0, 400.0, 0.92, 0.92, 400.0)]
EIGHT = [(20.0, 5.0, 10.0, 0.9, 0.95, 10.0), (3.0, 4.0, 8.0, 1.0, 1.0, 0.0), (10.0, 6.0, 30.0, 0.85, 0.8, 15.0), (0.0, 7.0, 20.0, 1.0, 0.9, 20.0),
         (5.0, 0.0, 10.0, 0.9, 0.9, 5.0), (2.0, 3.0, 0.0, 0.7, 0.7, 0.0), (6.0, 8.0, 24.0, 0.95, 0.95, 24.0), (50.0, 50.0, 12.5, 0.5, 0.5, 0.0)]


def _rts24():
    gens, load = hl1.rts24_generators(), hl1.rts24_load()
    return (np.array([g.capacity for g in gens]), np.array([g.mttf for g in gens]), np.array([g.mttr for g in gens]), load.hourly_load)


def _fleet(name):
    if name == "day":                              # fleet100 against 24 hours cut from its 1000-hour curve: several years inside one 64-step group
        cap, mttf, mttr, load = M.fleet100(1000)
        return cap, mttf, mttr, 1.0625 * load[162:186]        # the day at the crest of the slow component, raised so that hours are short
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
    eng._check(eng.L.relmc_hl1_seq(eng._h, seed, first, n, years, start, C.byref(acc), yr.ctypes.data_as(C.POINTER(_abi.Hl1SeqYear))),
               "relmc_hl1_seq")
    return acc, yr


def _sweep_level(eng, seed, first, n, years, start, scale, shift):
    arr = (_abi.Hl1SweepLevel * 1)(_abi.Hl1SweepLevel(scale, shift, 0, 0))
    acc = (_abi.Hl1SeqAcc * 1)()
    yr = np.zeros((n * years, 3))
    eng._check(eng.L.relmc_hl1_seq_sweep(eng._h, seed, first, n, years, start, 1, arr, None, acc, yr.ctypes.data_as(C.POINTER(_abi.Hl1SeqYear))),
               "relmc_hl1_seq_sweep")
    return yr


def _storage(eng, seed, first, n, years, start, storages, scale=1.0, shift=0.0, h=None, n_storage=None):
    """-> (acc, yr[n * years, 3], sy[n * years, 3], rc); storages: tuples of the six fields."""
    ns = len(storages)
    arr = (_abi.Hl1Storage * max(ns, 1))(*[_abi.Hl1Storage(*s) for s in storages])
    acc = _abi.Hl1StorageAcc()
    yr, sy = np.zeros((max(n * years, 0), 3)), np.zeros((max(n * years, 0), 3))
    rc = eng.L.relmc_hl1_seq_storage(h or eng._h, seed, first, n, years, start, scale, shift, ns if n_storage is None else n_storage,
                                     arr if ns else None, C.byref(acc), yr.ctypes.data_as(C.POINTER(_abi.Hl1SeqYear)),
                                     sy.ctypes.data_as(C.POINTER(_abi.Hl1StorageYear)))
    if h is None:
        eng._check(rc, "relmc_hl1_seq_storage")
    return acc, yr, sy, rc


def _acc_tuple(a):
    return tuple(getattr(a, f) for f in ACC_FIELDS)


@pytest.mark.gpu
@pytest.mark.parametrize("start", [M.ALL_UP, M.STATIONARY])
@pytest.mark.parametrize("fleet", ["rts24", "1000"])
def test_no_effect_is_bitwise(engine, fleet, start):
    """Chains 2 .. 6 (an offset range, a chain count that is no multiple of 4), 3 years each: without storages, and with storages that
    cannot act, the year records are relmc_hl1_seq's and relmc_hl1_seq_sweep's byte for byte; what cannot serve has an all-zero record."""
    _load(engine, *_fleet(fleet))
    args = (11, 2, 5, 3, start)
    _, ref = _seq(engine, *args)
    assert ref[:, 0].sum() > 0
    acc, yr, sy, _ = _storage(engine, *args, [])
    assert yr.tobytes() == ref.tobytes() and not sy.any()
    assert acc.years == 15 and acc.sum_lole == ref[:, 0].sum() and acc.sum_served == 0.0
    lvl = _sweep_level(engine, *args, 1.07, 33.25)
    assert lvl[:, 0].sum() > ref[:, 0].sum()
    _, yr, sy, _ = _storage(engine, *args, [], scale=1.07, shift=33.25)
    assert yr.tobytes() == lvl.tobytes() and not sy.any()
    no_discharge = [(50.0, 0.0, 200.0, 0.9, 0.9, 200.0), (50.0, 0.0, 100.0, 0.9, 0.9, 40.0)]      # the second one charges, and never delivers
    empty_no_charge = [(0.0, 50.0, 200.0, 0.9, 0.9, 0.0)] * 3
    no_energy = [(50.0, 50.0, 0.0, 0.9, 0.9, 0.0)] * 8
    for st, all_zero in ((no_discharge, False), (empty_no_charge, True), (no_energy, True)):
        for level, want in (((1.0, 0.0), ref), ((1.07, 33.25), lvl)):
            _, yr, sy, _ = _storage(engine, *args, st, scale=level[0], shift=level[1])
            assert yr.tobytes() == want.tobytes(), (st, level)
            assert not sy[:, :2].any() and (not sy.any() if all_zero else sy[:, 2].sum() > 0), (st, level)


_MODEL_SHAPES = {"small": (SMALL_STORAGES, 8, 3), "513": (F513_STORAGES, 4, 3), "day": (DAY_STORAGES, 6, 6), "rts24": (BATTERY, 8, 1)}


def _against_model(engine, fleet, storages, n, years, start, seed=7, first=0):
    cap, mttf, mttr, load = _fleet(fleet)
    _load(engine, cap, mttf, mttr, load)
    acc, yr, sy, _ = _storage(engine, seed, first, n, years, start, storages)
    rec, cnt = SM.storage_model(seed, range(first, first + n), cap, mttf, mttr, load, years, start, storages)
    np.testing.assert_array_equal(yr[:, 0], rec[:, 0])
    np.testing.assert_array_equal(yr[:, 2], rec[:, 2])
    np.testing.assert_array_equal(sy[:, 0], rec[:, 3])
    np.testing.assert_allclose(yr[:, 1], rec[:, 1], rtol=1e-12, atol=0.0)
    np.testing.assert_allclose(sy[:, 1], rec[:, 4], rtol=1e-12, atol=0.0)
    np.testing.assert_allclose(sy[:, 2], rec[:, 5], rtol=1e-12, atol=0.0)
    both = np.concatenate([yr, sy], axis=1)
    assert acc.years == n * years
    for q, f in enumerate(("sum_lole", "sum_eue", "sum_lolf", "sum_served", "sum_discharged", "sum_charged")):
        assert getattr(acc, f) == pytest.approx(both[:, q].sum(), rel=1e-12), f
        assert getattr(acc, f + "2") == pytest.approx((both[:, q] ** 2).sum(), rel=1e-12), f
    return rec, cnt


@pytest.mark.gpu
@pytest.mark.parametrize("start", [M.ALL_UP, M.STATIONARY])
@pytest.mark.parametrize("fleet", list(_MODEL_SHAPES))
def test_records_equal_the_host_model(engine, fleet, start):
    """Counts exact, energies to rel 1e-12 (the device sums lane partials, the model in step order), acc against its year records.
    small: a 168-hour year (three years inside one window); 513: a year one step longer than a window, two units per lane, all four
    mask words; day: a 24-hour year (several years inside one 64-step group); rts24: 17 windows of one year with the 100 MW battery."""
    storages, n, years = _MODEL_SHAPES[fleet]
    rec, cnt = _against_model(engine, fleet, storages, n, years, start)
    assert cnt["short"] > 0 and cnt["long"] > 0
    if fleet != "rts24":                           # 8 chain years of RTS-24 have a handful of short hours: the battery may serve all of them
        assert cnt["served"] > 0 and cnt["lost"] > 0 and rec[:, 5].sum() > 0


@pytest.mark.gpu
def test_eight_storages_equal_the_host_model(engine):
    """Eight unlike storages (one that cannot charge, one that cannot discharge, one without energy, lossy and lossless ones)."""
    rec, cnt = _against_model(engine, "small", EIGHT, 8, 3, M.STATIONARY)
    assert all(cnt["discharge"][i] > 0 for i in (0, 1, 2, 3, 6, 7)) and cnt["discharge"][4] == cnt["discharge"][5] == 0
    assert cnt["served"] > 0 and cnt["lost"] > 0 and cnt["clamp"] >= 0


@pytest.mark.gpu
@pytest.mark.parametrize("start", [M.ALL_UP, M.STATIONARY])
def test_invariants(engine, start):
    """served + lole is the no-storage lole year by year; a storage that can always deliver everything leaves no loss."""
    _load(engine, *_fleet("513"))
    args = (7, 1, 6, 3, start)
    _, ref = _seq(engine, *args)
    assert ref[:, 0].sum() > 0
    _, yr, sy, _ = _storage(engine, *args, F513_STORAGES)
    assert 0 < yr[:, 0].sum() < ref[:, 0].sum()
    np.testing.assert_array_equal((yr[:, 0] + sy[:, 0]).astype(np.int64), ref[:, 0].astype(np.int64))
    assert np.all(yr[:, 1] <= ref[:, 1]) and np.all(yr[:, 2] <= ref[:, 0])
    _, yr, sy, _ = _storage(engine, *args, [(1e9, 1e9, 1e9, 1.0, 1.0, 1e9)])
    assert not yr.any()
    np.testing.assert_array_equal(sy[:, 0].astype(np.int64), ref[:, 0].astype(np.int64))
    np.testing.assert_allclose(sy[:, 1], ref[:, 1], rtol=1e-12)          # everything short was delivered


@pytest.mark.gpu
def test_hand_pattern_on_the_device(engine):
    """The pattern of tests/test_hl1_storage_host.py (every number dyadic): one 100 MW unit whose first failure lies beyond the chain."""
    curve, storage, _, _, want = SM.hand_pattern()
    _load(engine, [100.0], [1e15], [1.0], curve)
    for first, n in ((0, 1), (5, 6)):
        acc, yr, sy, _ = _storage(engine, 3, first, n, 2, M.ALL_UP, [storage])
        np.testing.assert_array_equal(np.concatenate([yr, sy], axis=1), np.tile(want, (n, 1)))
        assert _acc_tuple(acc)[:4] == (2 * n, 8.0 * n, 73.0 * n, 3.0 * n) and (acc.sum_served, acc.sum_discharged, acc.sum_charged) == (4.0 * n, 47.0 * n, 64.0 * n)
    _, yr, sy, _ = _storage(engine, 3, 0, 1, 2, M.ALL_UP, [])
    np.testing.assert_array_equal(yr, [[6.0, 60.0, 3.0], [6.0, 60.0, 2.0]])


@pytest.mark.gpu
def test_split_and_repeat(engine):
    _load(engine, *_fleet("513"))
    args = (9, 3, 11, 3, M.STATIONARY)
    acc, yr, sy, _ = _storage(engine, *args, F513_STORAGES, shift=5.5)
    acc2, yr2, sy2, _ = _storage(engine, *args, F513_STORAGES, shift=5.5)
    assert yr.tobytes() == yr2.tobytes() and sy.tobytes() == sy2.tobytes() and _acc_tuple(acc) == _acc_tuple(acc2)
    a, ya, sa, _ = _storage(engine, 9, 3, 6, 3, M.STATIONARY, F513_STORAGES, shift=5.5)
    b, yb, sb, _ = _storage(engine, 9, 9, 5, 3, M.STATIONARY, F513_STORAGES, shift=5.5)
    assert np.concatenate([ya, yb]).tobytes() == yr.tobytes() and np.concatenate([sa, sb]).tobytes() == sy.tobytes()
    assert a.years + b.years == acc.years == 33
    for f in ("sum_lole", "sum_lolf", "sum_served", "sum_lole2", "sum_lolf2", "sum_served2"):
        assert getattr(a, f) + getattr(b, f) == getattr(acc, f), f
    assert yr[:, 0].sum() > 0 and sy[:, 0].sum() > 0


@pytest.mark.gpu
def test_error_codes(engine):
    L = engine.L
    h = C.c_void_p()
    assert L.relmc_ctx_create(0, C.byref(h)) == 0
    try:
        ok = [(20.0, 20.0, 60.0, 0.9, 0.95, 60.0), (10.0, 15.0, 30.0, 0.85, 1.0, 0.0)]
        run = lambda st=ok, n=4, years=2, start=0, **kw: _storage(engine, 1, 0, n, years, start, st, h=h, **kw)
        err = lambda: L.relmc_last_error(h).decode()
        assert run()[3] == -5                                                            # RELMC_ERR_NO_CASE
        assert _load(engine, *_fleet("small"), h=h) == 0
        good = run()
        assert good[3] == 0 and good[0].years == 8 and good[0].sum_served > 0
        nan, inf = float("nan"), float("inf")
        fields = ("charge_mw", "discharge_mw", "energy_mwh", "eta_charge", "eta_discharge", "soc0_mwh")

        def with_field(q, v):
            s = list(ok[1]); s[q] = v
            return [ok[0], tuple(s)]

        for q, name in enumerate(fields):                                                # every field, non-finite
            for v in (nan, inf, -inf):
                assert run(st=with_field(q, v))[3] == -1 and "storage 1" in err() and name in err(), (name, v, err())
        for q in range(3):                                                               # a negative power or energy
            assert run(st=with_field(q, -1.0))[3] == -1 and "storage 1" in err() and fields[q] in err(), err()
        for q in (3, 4):                                                                 # an efficiency outside (0, 1]
            for v in (0.0, -0.5, 1.0 + 2.0 ** -52):
                assert run(st=with_field(q, v))[3] == -1 and "storage 1" in err() and fields[q] in err(), err()
        for v in (-2.0 ** -60, 30.0 + 2.0 ** -40):                                       # soc0 outside [0, energy]
            assert run(st=with_field(5, v))[3] == -1 and "storage 1" in err() and "soc0_mwh" in err(), err()
        assert run(st=with_field(5, 30.0))[3] == 0 and run(st=with_field(3, 1.0))[3] == 0     # the edges are inside
        assert run(st=ok * 4 + ok[:1])[3] == -1 and "n_storage" in err()                 # nine
        assert run(st=[], n_storage=-1)[3] == -1 and "n_storage" in err()
        assert run(st=[], n_storage=2)[3] == -1 and "storage" in err()                   # a count without the array
        assert run(st=ok * 4)[3] == 0 and run(st=[])[3] == 0
        for kw in (dict(scale=nan), dict(shift=inf), dict(scale=-inf)):
            assert run(**kw)[3] == -1 and "scale / shift" in err(), kw
        assert run(start=2)[3] == -1 and run(start=-1)[3] == -1 and run(years=0)[3] == -1 and run(n=-1)[3] == -1
        arr = (_abi.Hl1Storage * 1)(_abi.Hl1Storage(*ok[0]))
        acc = _abi.Hl1StorageAcc()
        assert L.relmc_hl1_seq_storage(None, 1, 0, 4, 1, 0, 1.0, 0.0, 1, arr, C.byref(acc), None, None) == -1
        assert L.relmc_hl1_seq_storage(h, 1, 0, 4, 1, 0, 1.0, 0.0, 1, arr, None, None, None) == -1
        assert L.relmc_hl1_seq_storage(h, 1, 0, 4, 1, 0, 1.0, 0.0, 1, arr, C.byref(acc), None, None) == 0 and acc.years == 4   # both records optional
        # a refused call changes nothing
        acc.years, acc.sum_lole, acc.sum_charged2 = -7, 3.5, 2.5
        yr, sy = np.full((8, 3), -7.0), np.full((8, 3), -7.0)
        bad = (_abi.Hl1Storage * 2)(_abi.Hl1Storage(*ok[0]), _abi.Hl1Storage(10.0, 15.0, 30.0, 0.85, 1.0, 31.0))
        assert L.relmc_hl1_seq_storage(h, 1, 0, 4, 2, 0, 1.0, 0.0, 2, bad, C.byref(acc), yr.ctypes.data_as(C.POINTER(_abi.Hl1SeqYear)),
                                       sy.ctypes.data_as(C.POINTER(_abi.Hl1StorageYear))) == -1
        assert (acc.years, acc.sum_lole, acc.sum_charged2) == (-7, 3.5, 2.5) and np.all(yr == -7.0) and np.all(sy == -7.0)
        # n_chains == 0 zeroes the outputs
        assert L.relmc_hl1_seq_storage(h, 1, 0, 0, 2, 0, 1.0, 0.0, 1, arr, C.byref(acc), None, None) == 0
        assert _acc_tuple(acc) == (0,) + (0.0,) * 12
        # the refused calls left the model alone
        again = run()
        assert again[3] == 0 and again[1].tobytes() == good[1].tobytes() and again[2].tobytes() == good[2].tobytes()
    finally:
        L.relmc_ctx_destroy(h)


@pytest.fixture(scope="module")
def small_model():
    cap, mttf, mttr, load = M.small_fleet()
    return [hl1.Generator(i + 1, float(cap[i]), float(mttf[i]), float(mttr[i])) for i in range(cap.size)], hl1.LoadModel(load)


@pytest.mark.gpu
def test_python_run_and_report(engine, small_model):
    gens, load = small_model
    kw = dict(seed=5, chains=2000, start="stationary", engine=engine)
    base = hl1.run_sequential_mc(gens, load, 2000, **kw)
    none = hl1_storage.run_sequential_storage(gens, load, [], 2000, **kw)
    for f in ("year_lole", "year_eue", "year_lolf"):
        assert getattr(none, f).tobytes() == getattr(base, f).tobytes(), f
    assert (none.lole_hours_yr, none.eue_mwh_yr, none.lolf_occ_yr) == (base.lole_hours_yr, base.eue_mwh_yr, base.lolf_occ_yr)
    assert none.served_hours_yr == 0.0 and not none.year_charged.any()
    st = [hl1_storage.Storage(*s[:5], soc0_mwh=s[5]) for s in SMALL_STORAGES]
    res = hl1_storage.run_sequential_storage(gens, load, st, 2000, **kw)
    assert 0 < res.lole_hours_yr < base.lole_hours_yr and res.eue_mwh_yr < base.eue_mwh_yr
    np.testing.assert_array_equal(res.year_lole + res.year_served, base.year_lole)
    assert res.served_hours_yr == pytest.approx(base.lole_hours_yr - res.lole_hours_yr, rel=1e-12)
    assert 0 < res.discharged_mwh_yr < res.charged_mwh_yr                      # round-trip losses; both storages end no fuller than they may start
    txt = hl1_storage.storage_report(base, res)
    assert "2 storages:" in txt and ("%.4f" % res.lole_hours_yr) in txt
    full = hl1_storage.run_sequential_storage(gens, load, [hl1_storage.Storage(20.0, 20.0, 60.0)], 2000, **kw)     # soc0_mwh None: full
    same = hl1_storage.run_sequential_storage(gens, load, [(20.0, 20.0, 60.0, 1.0, 1.0, 60.0)], 2000, **kw)
    assert full.year_eue.tobytes() == same.year_eue.tobytes() and full.lole_hours_yr < base.lole_hours_yr


@pytest.mark.gpu
@pytest.mark.parametrize("metric", ["lole", "eue"])
def test_python_storage_elcc(engine, small_model, metric):
    gens, load = small_model
    kw = dict(seed=5, chains=2000, start="stationary", engine=engine)
    st = [hl1_storage.Storage(20.0, 20.0, 60.0, 0.9, 0.95)]
    r = hl1_storage.storage_elcc(gens, load, st, 2000, metric=metric, **kw)
    base = hl1.run_sequential_mc(gens, load, 2000, **kw)
    attr = hl1._SWEEP_METRIC[metric]
    assert r.target == getattr(base, attr) and r.rounds == 3 and r.mode == "shift"
    assert 0.0 <= r.pair[0] <= r.value <= r.pair[1] <= 20.0
    assert r.pair[1] - r.pair[0] == pytest.approx(20.0 / 7 ** 3, rel=1e-9)
    assert min(r.pair_metric) <= r.target <= max(r.pair_metric)
    assert 0 < r.std_error < 20.0
    at = hl1_storage.run_sequential_storage(gens, load, st, 2000, shift=r.value, **kw)
    assert min(r.pair_metric) <= getattr(at, attr) <= max(r.pair_metric)
    two = hl1_storage.storage_elcc(gens, load, st + [hl1_storage.Storage(10.0, 15.0, 30.0, 0.85, 1.0, 0.0)], 2000, metric=metric, rounds=2, **kw)
    assert r.value < two.value <= 35.0 and min(two.pair_metric) <= two.target <= max(two.pair_metric)
