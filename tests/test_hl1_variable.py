"""Weather-year wind and solar resources on the HL1 sequential chronology on the GPU (relmc_hl1_var_load, relmc_hl1_var_seq): the three
bitwise pins of the contract against relmc_hl1_seq, relmc_hl1_seq_storage and relmc_hl1_seq_sweep, the [w][r][h] indexing against
relmc_hl1_seq under CYCLE, the host model (tests/tools/hl1_variable_model.py) on shapes that put several years and weather years into
one 64-step group, the invariants, split / repeat invariance, an exact expectation, the error codes, and the Python layer of
hl1_variable.py."""
import ctypes as C
import functools
import importlib.util
import os

import numpy as np
import pytest

from powersystemsreliabilityassessment_amd import _abi, hl1, hl1_storage, hl1_variable

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("hl1_variable_model", os.path.join(ROOT, "tests", "tools", "hl1_variable_model.py"))
VM = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(VM)
SM, M = VM.SM, VM.SEQ

dp = _abi.c_double_p
ACC_FIELDS = [f for f, _ in _abi.Hl1StorageAcc._fields_]
RANDOM, CYCLE = VM.PICK_RANDOM, VM.PICK_CYCLE
# (charge_mw, discharge_mw, energy_mwh, eta_charge, eta_discharge, soc0_mwh); the sets of tests/test_hl1_storage.py
SMALL_STORAGES = [(20.0, 20.0, 60.0, 0.9, 0.95, 60.0), (10.0, 15.0, 30.0, 0.85, 1.0, 0.0)]
F513_STORAGES = [(30.0, 30.0, 90.0, 0.9, 0.9, 90.0), (15.0, 25.0, 40.0, 0.8, 1.0, 0.0)]
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
        return cap, mttf, mttr, 1.0625 * load[162:186]
    return _rts24() if name == "rts24" else M.small_fleet() if name == "small" else M.fleet100(int(name))


def _weather(load, n_weather, n_res, seed, curves, share=0.02):
    """A deterministic library for the load curve `load`: resource r gives 0 .. share * (r + 1) * mean load, rounded to 1/64 MW; a weather
    year's own load curve is `load` times 0.97 .. 1.03."""
    rng = np.random.default_rng(seed)
    load = np.asarray(load, dtype=np.float64)
    top = share * load.mean() * (np.arange(n_res) + 1.0)
    out = np.round(rng.uniform(0.0, 1.0, (n_weather, n_res, load.size)) * top[None, :, None] * 64.0) / 64.0
    wl = load[None, :] * np.linspace(0.97, 1.03, n_weather)[:, None] if curves else None
    return out, wl


def _load(eng, cap, mttf, mttr, load, h=None):
    arrs = [np.ascontiguousarray(x, dtype=np.float64) for x in (cap, mttf, mttr, load)]
    rc = eng.L.relmc_hl1_seq_load(h or eng._h, arrs[0].size, *[a.ctypes.data_as(dp) for a in arrs[:3]], arrs[3].size, arrs[3].ctypes.data_as(dp))
    if h is None:
        eng._check(rc, "relmc_hl1_seq_load")
        eng._hl1_seq_loaded = None                 # hl1's cache no longer describes the device
    return rc


def _var_load(eng, out, wl=None, h=None, shape=None):
    out = np.ascontiguousarray(out, dtype=np.float64)
    nw, nres, H = shape or out.shape
    wl = None if wl is None else np.ascontiguousarray(wl, dtype=np.float64)
    rc = eng.L.relmc_hl1_var_load(h or eng._h, nw, nres, H, out.ctypes.data_as(dp) if out.size else None, None if wl is None else wl.ctypes.data_as(dp))
    if h is None:
        eng._check(rc, "relmc_hl1_var_load")
        eng._hl1_var_loaded = None                 # hl1_variable's cache no longer describes the device
    return rc


def _opts(rs=(), scale=1.0, shift=0.0, pick=RANDOM, reserved=0):
    o = _abi.Hl1VarOpts()
    for r, v in enumerate(rs):
        o.resource_scale[r] = v
    o.scale, o.shift, o.pick, o.reserved = scale, shift, pick, reserved
    return o


def _var(eng, seed, first, n, years, start, storages=(), rs=(), scale=1.0, shift=0.0, pick=RANDOM, h=None, n_storage=None, opts=None):
    """-> (acc, yr[n * years, 3], sy[n * years, 3], weather[n * years], rc); storages: tuples of the six fields."""
    ns = len(storages)
    arr = (_abi.Hl1Storage * max(ns, 1))(*[_abi.Hl1Storage(*s) for s in storages])
    acc = _abi.Hl1StorageAcc()
    m = max(n * years, 0)
    yr, sy, wy = np.zeros((m, 3)), np.zeros((m, 3)), np.full(m, -1, dtype=np.int32)
    o = opts if opts is not None else _opts(rs, scale, shift, pick)
    rc = eng.L.relmc_hl1_var_seq(h or eng._h, seed, first, n, years, start, C.byref(o), ns if n_storage is None else n_storage,
                                 arr if ns else None, C.byref(acc), yr.ctypes.data_as(C.POINTER(_abi.Hl1SeqYear)),
                                 sy.ctypes.data_as(C.POINTER(_abi.Hl1StorageYear)), wy.ctypes.data_as(_abi.c_int32_p))
    if h is None:
        eng._check(rc, "relmc_hl1_var_seq")
    return acc, yr, sy, wy, rc


def _seq(eng, seed, first, n, years, start):
    acc = _abi.Hl1SeqAcc()
    yr = np.zeros((n * years, 3))
    eng._check(eng.L.relmc_hl1_seq(eng._h, seed, first, n, years, start, C.byref(acc), yr.ctypes.data_as(C.POINTER(_abi.Hl1SeqYear))), "relmc_hl1_seq")
    return yr


def _sweep_level(eng, seed, first, n, years, start, scale, shift):
    arr = (_abi.Hl1SweepLevel * 1)(_abi.Hl1SweepLevel(scale, shift, 0, 0))
    acc = (_abi.Hl1SeqAcc * 1)()
    yr = np.zeros((n * years, 3))
    eng._check(eng.L.relmc_hl1_seq_sweep(eng._h, seed, first, n, years, start, 1, arr, None, acc, yr.ctypes.data_as(C.POINTER(_abi.Hl1SeqYear))),
               "relmc_hl1_seq_sweep")
    return yr


def _storage(eng, seed, first, n, years, start, storages, scale=1.0, shift=0.0):
    ns = len(storages)
    arr = (_abi.Hl1Storage * max(ns, 1))(*[_abi.Hl1Storage(*s) for s in storages])
    acc = _abi.Hl1StorageAcc()
    yr, sy = np.zeros((n * years, 3)), np.zeros((n * years, 3))
    eng._check(eng.L.relmc_hl1_seq_storage(eng._h, seed, first, n, years, start, scale, shift, ns, arr if ns else None, C.byref(acc),
                                           yr.ctypes.data_as(C.POINTER(_abi.Hl1SeqYear)), sy.ctypes.data_as(C.POINTER(_abi.Hl1StorageYear))),
               "relmc_hl1_seq_storage")
    return acc, yr, sy


def _acc_tuple(a):
    return tuple(getattr(a, f) for f in ACC_FIELDS)


@pytest.mark.gpu
@pytest.mark.parametrize("start", [M.ALL_UP, M.STATIONARY])
@pytest.mark.parametrize("fleet", ["rts24", "1000"])
def test_pins_1_and_2_are_bitwise(engine, fleet, start):
    """Chains 2 .. 6 (an offset range, a chain count that is no multiple of 4), 3 years each, both picks, without and with SMALL_STORAGES.
    Pin 1: no resource, or every resource scaled 0, and no load curves -> relmc_hl1_seq_storage's two rows (and relmc_hl1_seq's at
    (1, 0) without storage).  Pin 2: one weather year with the load curve X and no effective resource -> relmc_hl1_seq_storage on the
    model loaded with X."""
    cap, mttf, mttr, load = _fleet(fleet)
    _load(engine, cap, mttf, mttr, load)
    args = (11, 2, 5, 3, start)
    ref = _seq(engine, *args)
    assert ref[:, 0].sum() > 0
    want = {(st, lv): _storage(engine, *args, list(st), *lv) for st in ((), tuple(SMALL_STORAGES)) for lv in ((1.0, 0.0), (1.07, 33.25))}
    assert want[(), (1.0, 0.0)][1].tobytes() == ref.tobytes()
    assert want[tuple(SMALL_STORAGES), (1.07, 33.25)][2][:, 2].sum() > 0                # the storages act: the empty one charges
    out, _ = _weather(load, 3, 2, 3, False)
    for lib, rs in ((np.zeros((3, 0, load.size)), ()), (out, (0.0, 0.0))):
        _var_load(engine, lib)
        for pick in (RANDOM, CYCLE):
            for (st, lv), (wa, wy_, ws) in want.items():
                acc, yr, sy, wy, _ = _var(engine, *args, list(st), rs, lv[0], lv[1], pick)
                assert yr.tobytes() == wy_.tobytes() and sy.tobytes() == ws.tobytes(), (rs, pick, lv, len(st))
                assert _acc_tuple(acc) == _acc_tuple(wa)
                assert wy.min() >= 0 and wy.max() <= 2
    # pin 2
    X = 1.07 * load + 33.25
    _var_load(engine, out[:1], X[None, :])
    got = {(st, pick): _var(engine, *args, list(st), (0.0, 0.0), 1.0, 0.0, pick) for st in ((), tuple(SMALL_STORAGES)) for pick in (RANDOM, CYCLE)}
    _load(engine, cap, mttf, mttr, X)
    for (st, pick), (acc, yr, sy, wy, _) in got.items():
        wa, wy_, ws = _storage(engine, *args, list(st))
        assert yr.tobytes() == wy_.tobytes() and sy.tobytes() == ws.tobytes() and _acc_tuple(acc) == _acc_tuple(wa), (pick, len(st))
        assert not wy.any()
        assert yr.tobytes() == want[st, (1.07, 33.25)][1].tobytes()          # X is the raised level's curve, rounded the same way


def _dyadic_small():
    cap, mttf, mttr, load = M.small_fleet()
    return cap, mttf, mttr, np.round(load * 8.0) / 8.0


@pytest.mark.gpu
@pytest.mark.parametrize("start", [M.ALL_UP, M.STATIONARY])
def test_pin_3_constant_resource_is_a_load_shift(engine, start):
    """small_fleet (integer capacities) with its load rounded to multiples of 0.125 and one resource of constant p = 12.5 MW: every sum is
    exact, so the records are relmc_hl1_seq_sweep's level (scale, shift - p, fleet 0), bit for bit."""
    cap, mttf, mttr, load = _dyadic_small()
    _load(engine, cap, mttf, mttr, load)
    _var_load(engine, np.full((3, 1, load.size), 12.5))
    args = (11, 2, 5, 3, start)
    for scale, shift in ((1.0, 4.0), (1.25, -20.0)):
        lvl = _sweep_level(engine, *args, scale, shift - 12.5)
        base = _sweep_level(engine, *args, scale, shift)
        assert 0 < lvl[:, 0].sum() < base[:, 0].sum()
        for pick in (RANDOM, CYCLE):
            _, yr, sy, _, _ = _var(engine, *args, [], (1.0,), scale, shift, pick)
            assert yr.tobytes() == lvl.tobytes() and not sy.any()
            _, yr, _, _, _ = _var(engine, *args, [], (0.0,), scale, shift, pick)
            assert yr.tobytes() == base.tobytes()


@pytest.mark.gpu
def test_cycle_is_the_sequential_model_on_each_weather_years_net_load(engine):
    """years_per_chain = 1, three weather years with their own load curves, two resources, dyadic data, no storage: chain c's record is
    chain c's record of relmc_hl1_seq on the model loaded with load_w - v_w, w = c mod 3, bit for bit.  A wrong [w][r][h] index shows here."""
    cap, mttf, mttr, load = _dyadic_small()
    rng = np.random.default_rng(17)
    out = np.round(rng.uniform(0.0, 24.0, (3, 2, load.size)) * 4.0) / 4.0
    wl = np.stack([load, load + 6.5, load - 3.25])
    rs = (0.5, 1.0)
    _load(engine, cap, mttf, mttr, load)
    _var_load(engine, out, wl)
    first, n = 1, 31
    _, yr, sy, wy, _ = _var(engine, 5, first, n, 1, M.STATIONARY, [], rs, pick=CYCLE)
    assert wy.tolist() == [(first + c) % 3 for c in range(n)] and not sy.any()
    for w in range(3):
        net = wl[w] - (rs[0] * out[w, 0] + rs[1] * out[w, 1])
        _load(engine, cap, mttf, mttr, net)
        ref = _seq(engine, 5, first, n, 1, M.STATIONARY)
        sel = wy == w
        assert sel.sum() >= 2 and yr[sel].tobytes() == ref[sel].tobytes(), w
        assert ref[sel, 0].sum() > 0
    assert len({yr[wy == w].tobytes() for w in range(3)}) == 3


# name: fleet, chains, years, n_weather, n_resources, resource scales, pick, start, load curves, storages, scale, shift
_CASES = {
    "day-2res-curves-2st":    ("day", 6, 6, 3, 2, (1.0, 0.5), RANDOM, M.STATIONARY, True, DAY_STORAGES, 1.0, 0.0),
    "day-8res-one-off-0st":   ("day", 6, 6, 3, 8, (0.25, 0.0, 0.125, 0.25, 0.125, 0.25, 0.125, 0.125), CYCLE, M.ALL_UP, False, [], 1.0, 0.0),
    "130-1res-curves-8st":    ("130", 4, 3, 3, 1, (1.0,), RANDOM, M.ALL_UP, True, EIGHT, 1.0, 0.0),
    "513-2res-1w-2st":        ("513", 4, 3, 1, 2, (1.0, 1.0), CYCLE, M.STATIONARY, False, F513_STORAGES, 1.0, 0.0),
    "small-2res-curves-8st":  ("small", 8, 3, 3, 2, (1.0, 0.75), CYCLE, M.STATIONARY, True, EIGHT, 1.0, 0.0),
    "small-2res-0st":         ("small", 8, 3, 3, 2, (1.0, 0.0), RANDOM, M.ALL_UP, True, [], 1.0, 0.0),
    "rts24-2res-curves-1st":  ("rts24", 8, 1, 3, 2, (1.0, 1.0), RANDOM, M.STATIONARY, True, BATTERY, 1.0, 0.0),
}
_CASE_SHARE = {"rts24": 0.05}
_CASE_SHIFT = {}


@functools.lru_cache(maxsize=None)
def _case(name):
    """The data and the host model's records of a case, computed once."""
    fleet, n, years, nw, nres, rs, pick, start, curves, storages, scale, shift = _CASES[name]
    cap, mttf, mttr, load = _fleet(fleet)
    out, wl = _weather(load, nw, nres, 23, curves, _CASE_SHARE.get(fleet, 0.02))
    cnt = SM.new_counters()
    rec, wy = VM.variable_model(7, range(n), cap, mttf, mttr, load, years, start, out, wl, rs, pick, storages, scale, shift, cnt)
    rec.setflags(write=False)
    return (cap, mttf, mttr, load), out, wl, rec, wy, cnt


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(_CASES))
def test_records_equal_the_host_model(engine, name):
    """Counts exact, energies to rel 1e-12 (the device sums lane partials, the model in step order; the tolerance of
    tests/test_hl1_storage.py), weather_host equal to the model's weather years, acc against its year records.  day: a 24-hour year
    (several years and weather years inside one 64-step group); 130: the year edge moves two lanes a year; 513: a year one step longer
    than a window, two units per lane; small: a 168-hour year; rts24: 17 windows of one year.  Every case reaches short and long steps
    and both quiet groups and the serial stage; the cases with storages reach served, lost, charging and discharging steps too."""
    fleet, n, years, nw, nres, rs, pick, start, curves, storages, scale, shift = _CASES[name]
    model, out, wl, rec, wy_model, cnt = _case(name)
    _load(engine, *model)
    _var_load(engine, out, wl)
    acc, yr, sy, wy, _ = _var(engine, 7, 0, n, years, start, storages, rs, scale, shift, pick)
    np.testing.assert_array_equal(wy, wy_model)
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
    assert cnt["short"] > 0 and cnt["long"] > 0 and cnt["lost"] > 0 and 0 < cnt["serial_groups"] < cnt["groups"], cnt
    if nw > 1:
        assert np.unique(wy).size == nw
    if storages:
        assert cnt["served"] > 0 and sum(cnt["charge"]) > 0 and sum(cnt["discharge"]) > 0 and rec[:, 5].sum() > 0, cnt


@pytest.mark.gpu
@pytest.mark.parametrize("start", [M.ALL_UP, M.STATIONARY])
def test_invariants(engine, start):
    """served + lole is the no-storage lole of the same options, year by year; without storage LOLE and EUE do not rise with a resource's
    scale and do not fall with the shift, record by record (the fleet history and the weather years are the same)."""
    cap, mttf, mttr, load = _fleet("513")
    out, wl = _weather(load, 3, 2, 29, True)
    _load(engine, cap, mttf, mttr, load)
    _var_load(engine, out, wl)
    args = (7, 1, 6, 3, start)
    kw = dict(rs=(1.0, 0.5), shift=2.5)
    _, ref, zero, wy0, _ = _var(engine, *args, [], **kw)
    _, yr, sy, wy, _ = _var(engine, *args, F513_STORAGES, **kw)
    assert not zero.any() and np.array_equal(wy, wy0)
    assert 0 < yr[:, 0].sum() < ref[:, 0].sum()
    np.testing.assert_array_equal((yr[:, 0] + sy[:, 0]).astype(np.int64), ref[:, 0].astype(np.int64))
    assert np.all(yr[:, 1] <= ref[:, 1])
    rows = [_var(engine, *args, [], rs=s, shift=2.5)[1] for s in ((0.0, 0.0), (0.5, 0.0), (0.5, 0.5), (1.0, 0.5), (1.0, 3.0))]
    assert rows[3].tobytes() == ref.tobytes()
    for a, b in zip(rows, rows[1:]):
        assert np.all(a[:, 0] >= b[:, 0]) and np.all(a[:, 1] >= b[:, 1])
        assert a[:, 0].sum() > b[:, 0].sum()
    rows = [_var(engine, *args, [], rs=(1.0, 0.5), shift=s)[1] for s in (-10.0, 0.0, 2.5, 20.0)]
    for a, b in zip(rows, rows[1:]):
        assert np.all(a[:, 0] <= b[:, 0]) and np.all(a[:, 1] <= b[:, 1])
        assert a[:, 0].sum() < b[:, 0].sum()


@pytest.mark.gpu
@pytest.mark.parametrize("pick", [RANDOM, CYCLE])
def test_split_and_repeat(engine, pick):
    cap, mttf, mttr, load = _fleet("513")
    out, wl = _weather(load, 3, 2, 29, True)
    _load(engine, cap, mttf, mttr, load)
    _var_load(engine, out, wl)
    kw = dict(storages=F513_STORAGES, rs=(1.0, 0.5), shift=5.5, pick=pick)
    acc, yr, sy, wy, _ = _var(engine, 9, 3, 11, 3, M.STATIONARY, **kw)
    acc2, yr2, sy2, wy2, _ = _var(engine, 9, 3, 11, 3, M.STATIONARY, **kw)
    assert yr.tobytes() == yr2.tobytes() and sy.tobytes() == sy2.tobytes() and _acc_tuple(acc) == _acc_tuple(acc2) and np.array_equal(wy, wy2)
    a, ya, sa, wa, _ = _var(engine, 9, 3, 6, 3, M.STATIONARY, **kw)
    b, yb, sb, wb, _ = _var(engine, 9, 9, 5, 3, M.STATIONARY, **kw)
    assert np.concatenate([ya, yb]).tobytes() == yr.tobytes() and np.concatenate([sa, sb]).tobytes() == sy.tobytes()
    assert np.array_equal(np.concatenate([wa, wb]), wy) and np.unique(wy).size == 3
    assert wy.tolist() == VM.weather_years(9, range(3, 14), 3, 3, pick).reshape(-1).tolist()
    assert a.years + b.years == acc.years == 33
    for f in ("sum_lole", "sum_lolf", "sum_served", "sum_lole2", "sum_lolf2", "sum_served2"):
        assert getattr(a, f) + getattr(b, f) == getattr(acc, f), f
    assert yr[:, 0].sum() > 0 and sy[:, 0].sum() > 0


def _expectation_case():
    cap, mttf, mttr, load = M.small_fleet()
    rng = np.random.default_rng(41)
    out = np.round(rng.uniform(0.0, 1.0, (3, 2, 168)) * np.array([12.0, 24.0])[None, :, None], 2)
    wl = np.round(load[None, :] * np.array([0.95, 1.025, 1.1])[:, None], 2)
    return cap, mttf, mttr, load, out, wl, (1.0, 0.5)


@pytest.mark.gpu
def test_exact_expectation(engine):
    """small_fleet, stationary start, CYCLE, 6000 one-year chains: every chain year is independent and the three weather years (with
    their own load curves, two resources) are equally weighted, 2000 chains each.  The expectation is the mean over w of
    hl1_seq_model.stationary_year against max(L_w - v_w, 0); the sampled LOLE and EUE lie within 4 standard errors of it (the standard
    error of the 6000 records), and the expectation without the resources lies more than 10 standard errors away, so the test cannot
    pass with the resources ignored.  The host model alone meets both conditions under this seed on chains 0 .. 1799."""
    cap, mttf, mttr, load, out, wl, rs = _expectation_case()
    _load(engine, cap, mttf, mttr, load)
    _var_load(engine, out, wl)
    n = 6000
    _, yr, _, wy, _ = _var(engine, 2026, 0, n, 1, M.STATIONARY, [], rs, pick=CYCLE)
    assert np.bincount(wy, minlength=3).tolist() == [2000, 2000, 2000]
    ci = cap.astype(int)
    want = np.mean([M.stationary_year(ci, mttf, mttr, np.maximum(wl[w] - (rs[0] * out[w, 0] + rs[1] * out[w, 1]), 0.0)) for w in range(3)], axis=0)
    bare = np.mean([M.stationary_year(ci, mttf, mttr, wl[w]) for w in range(3)], axis=0)
    for q, name in ((0, "lole"), (1, "eue")):
        mean, se = yr[:, q].mean(), yr[:, q].std(ddof=1) / np.sqrt(n)
        print(f"{name}: sampled {mean:.6g} +- {se:.3g}, exact {want[q]:.6g} (z {(mean - want[q]) / se:+.2f}), without resources {bare[q]:.6g} "
              f"({(bare[q] - mean) / se:.1f} se away)")
        assert abs(mean - want[q]) < 4.0 * se, name
        assert bare[q] - mean > 10.0 * se, name


@pytest.mark.gpu
def test_error_codes(engine):
    L = engine.L
    h = C.c_void_p()
    assert L.relmc_ctx_create(0, C.byref(h)) == 0
    try:
        cap, mttf, mttr, load = M.small_fleet()
        out, wl = _weather(load, 3, 2, 31, True)
        ok = list(SMALL_STORAGES)
        run = lambda st=ok, n=4, years=2, start=0, **kw: _var(engine, 1, 0, n, years, start, st, h=h, **{"rs": (1.0, 0.5), **kw})
        err = lambda: L.relmc_last_error(h).decode()
        nan, inf = float("nan"), float("inf")
        assert run()[4] == -5 and "relmc_hl1_seq_load" in err()                           # RELMC_ERR_NO_CASE before either load call
        assert _var_load(engine, out, wl, h=h) == 0
        assert run()[4] == -5 and "relmc_hl1_seq_load" in err()
        assert _load(engine, cap, mttf, mttr, load[:100], h=h) == 0
        assert run()[4] == -1 and "100" in err() and "168" in err()                       # the two nhours differ
        h2 = C.c_void_p()
        assert L.relmc_ctx_create(0, C.byref(h2)) == 0
        try:
            assert _load(engine, cap, mttf, mttr, load, h=h2) == 0
            assert _var(engine, 1, 0, 4, 2, 0, ok, (1.0, 0.5), h=h2)[4] == -5 and "relmc_hl1_var_load" in L.relmc_last_error(h2).decode()
        finally:
            L.relmc_ctx_destroy(h2)
        assert _load(engine, cap, mttf, mttr, load, h=h) == 0
        good = run()
        assert good[4] == 0 and good[0].years == 8 and good[0].sum_served > 0 and good[3].min() >= 0
        # relmc_hl1_var_load's refusals: each names what is wrong, and leaves the library alone
        def spoiled(a, idx, v):
            b = a.copy(); b[idx] = v
            return b
        for v, word in ((nan, "not finite"), (inf, "not finite"), (-0.5, "negative")):
            assert _var_load(engine, spoiled(out, (2, 1, 77), v), wl, h=h) == -1
            assert "weather year 2" in err() and "resource 1" in err() and "hour 77" in err() and word in err(), err()
        assert _var_load(engine, out, spoiled(wl, (1, 5), nan), h=h) == -1 and "weather year 1" in err() and "hour 5" in err() and "load" in err()
        assert _var_load(engine, out, spoiled(wl, (1, 5), -7.0), h=h) == 0 and _var_load(engine, out, wl, h=h) == 0        # a load may be negative
        for shape, word in (((0, 2, 168), "n_weather"), ((257, 2, 168), "n_weather"), ((3, -1, 168), "n_resources"), ((3, 9, 168), "n_resources"),
                            ((3, 2, 0), "nhours")):
            assert _var_load(engine, out, wl, h=h, shape=shape) == -1 and word in err(), shape
        assert L.relmc_hl1_var_load(h, 3, 2, 168, None, None) == -1 and "output_mw" in err()
        assert _var_load(engine, out, None, h=h, shape=(256, 8, 1 << 20)) == -4 and "2^31" in err()      # RELMC_ERR_UNSUPPORTED, before any value is read
        assert L.relmc_hl1_var_load(None, 3, 0, 168, None, None) == -1
        again = run()
        assert again[4] == 0 and again[1].tobytes() == good[1].tobytes() and again[2].tobytes() == good[2].tobytes()
        # relmc_hl1_var_seq's own refusals
        for rs, word in (((nan, 0.5), "resource_scale 0"), ((1.0, inf), "resource_scale 1"), ((1.0, -0.25), "resource_scale 1"),
                         ((1.0, 0.5, 0.125), "resource_scale 2"), ((1.0, 0.5, 0.0, 0.0, 0.0, 0.0, 0.0, 2.0), "resource_scale 7")):
            assert run(rs=rs)[4] == -1 and word in err(), (rs, err())
        assert run(rs=(0.0, 0.0))[4] == 0 and run(rs=(1.0,))[4] == 0
        for pick in (2, -1):
            assert run(pick=pick)[4] == -1 and "pick" in err()
        assert run(opts=_opts((1.0, 0.5), reserved=1))[4] == -1 and "reserved" in err()
        for kw in (dict(scale=nan), dict(shift=inf), dict(scale=-inf)):
            assert run(**kw)[4] == -1 and "scale / shift" in err(), kw
        assert run(start=2)[4] == -1 and run(start=-1)[4] == -1 and run(years=0)[4] == -1 and run(n=-1)[4] == -1
        # relmc_hl1_seq_storage's refusals
        fields = ("charge_mw", "discharge_mw", "energy_mwh", "eta_charge", "eta_discharge", "soc0_mwh")

        def with_field(q, v):
            s = list(ok[1]); s[q] = v
            return [ok[0], tuple(s)]

        for q, name in enumerate(fields):
            for v in (nan, inf):
                assert run(st=with_field(q, v))[4] == -1 and "storage 1" in err() and name in err(), (name, v, err())
        for q in range(3):
            assert run(st=with_field(q, -1.0))[4] == -1 and "storage 1" in err() and fields[q] in err(), err()
        for q in (3, 4):
            for v in (0.0, 1.0 + 2.0 ** -52):
                assert run(st=with_field(q, v))[4] == -1 and "storage 1" in err() and fields[q] in err(), err()
        for v in (-2.0 ** -60, 30.0 + 2.0 ** -40):
            assert run(st=with_field(5, v))[4] == -1 and "storage 1" in err() and "soc0_mwh" in err(), err()
        assert run(st=ok * 4 + ok[:1])[4] == -1 and "n_storage" in err()
        assert run(st=[], n_storage=-1)[4] == -1 and "n_storage" in err()
        assert run(st=[], n_storage=2)[4] == -1 and "storage" in err()
        assert run(st=ok * 4)[4] == 0 and run(st=[])[4] == 0
        o = _opts((1.0, 0.5))
        acc = _abi.Hl1StorageAcc()
        assert L.relmc_hl1_var_seq(None, 1, 0, 4, 1, 0, C.byref(o), 0, None, C.byref(acc), None, None, None) == -1
        assert L.relmc_hl1_var_seq(h, 1, 0, 4, 1, 0, C.byref(o), 0, None, None, None, None, None) == -1
        assert L.relmc_hl1_var_seq(h, 1, 0, 4, 1, 0, None, 0, None, C.byref(acc), None, None, None) == -1 and "opts" in err()
        assert L.relmc_hl1_var_seq(h, 1, 0, 4, 1, 0, C.byref(o), 0, None, C.byref(acc), None, None, None) == 0 and acc.years == 4    # every record optional
        # a refused call changes nothing
        acc.years, acc.sum_lole, acc.sum_charged2 = -7, 3.5, 2.5
        yr, sy, wy = np.full((8, 3), -7.0), np.full((8, 3), -7.0), np.full(8, -7, dtype=np.int32)
        bad = _opts((1.0, -1.0))
        assert L.relmc_hl1_var_seq(h, 1, 0, 4, 2, 0, C.byref(bad), 0, None, C.byref(acc), yr.ctypes.data_as(C.POINTER(_abi.Hl1SeqYear)),
                                   sy.ctypes.data_as(C.POINTER(_abi.Hl1StorageYear)), wy.ctypes.data_as(_abi.c_int32_p)) == -1
        assert (acc.years, acc.sum_lole, acc.sum_charged2) == (-7, 3.5, 2.5) and np.all(yr == -7.0) and np.all(sy == -7.0) and np.all(wy == -7)
        # n_chains == 0 zeroes the outputs
        assert L.relmc_hl1_var_seq(h, 1, 0, 0, 2, 0, C.byref(o), 0, None, C.byref(acc), None, None, None) == 0
        assert _acc_tuple(acc) == (0,) + (0.0,) * 12
        again = run()
        assert again[4] == 0 and again[1].tobytes() == good[1].tobytes() and again[2].tobytes() == good[2].tobytes() and np.array_equal(again[3], good[3])
    finally:
        L.relmc_ctx_destroy(h)


@pytest.fixture(scope="module")
def small_model():
    cap, mttf, mttr, load = _dyadic_small()
    return [hl1.Generator(i + 1, float(cap[i]), float(mttf[i]), float(mttr[i])) for i in range(cap.size)], hl1.LoadModel(load)


@pytest.mark.gpu
def test_python_run_and_report(engine, small_model):
    gens, load = small_model
    kw = dict(seed=5, chains=2000, start="stationary", engine=engine)
    base = hl1.run_sequential_mc(gens, load, 2000, **kw)
    out, _ = _weather(load.hourly_load, 3, 2, 37, False, share=0.05)
    W = hl1_variable.WeatherYears(out, None, ("a", "b"))
    for none in (hl1_variable.run_sequential_variable(gens, load, hl1_variable.WeatherYears(np.zeros((2, 0, 168))), 2000, **kw),
                 hl1_variable.run_sequential_variable(gens, load, W, 2000, resource_scale=(0.0, 0.0), pick="cycle", **kw)):
        for f in ("year_lole", "year_eue", "year_lolf"):
            assert getattr(none, f).tobytes() == getattr(base, f).tobytes(), f
        assert (none.lole_hours_yr, none.eue_mwh_yr, none.lolf_occ_yr) == (base.lole_hours_yr, base.eue_mwh_yr, base.lolf_occ_yr)
        assert none.served_hours_yr == 0.0 and not none.year_charged.any() and none.offered_mwh_yr == 0.0 and none.method == "Sequential MC"
    res = hl1_variable.run_sequential_variable(gens, load, W, 2000, **kw)
    assert 0 < res.lole_hours_yr < base.lole_hours_yr and res.eue_mwh_yr < base.eue_mwh_yr
    assert res.year_weather.shape == (2000,) and set(res.year_weather.tolist()) == {0, 1, 2}
    assert res.offered_mwh_yr == pytest.approx(out.sum(axis=(1, 2))[res.year_weather].mean(), rel=1e-12)
    st = [hl1_storage.Storage(*s[:5], soc0_mwh=s[5]) for s in SMALL_STORAGES]
    both = hl1_variable.run_sequential_variable(gens, load, W, 2000, storages=st, **kw)
    np.testing.assert_array_equal(both.year_lole + both.year_served, res.year_lole)
    assert 0 < both.lole_hours_yr < res.lole_hours_yr and both.charged_mwh_yr > 0 and np.array_equal(both.year_weather, res.year_weather)
    txt = hl1_variable.variable_report(base, both)
    assert "2 resources over 3 weather years drawn (random)" in txt and "2 storages:" in txt and ("%.4f" % both.lole_hours_yr) in txt
    print(txt)


@pytest.mark.gpu
def test_python_resource_elcc(engine, small_model):
    """A constant dyadic resource p = 12.5 on dyadic data is a load shift of -p exactly, so the metric at the shift p is the target bit for
    bit.  The sampled metric is a staircase in the shift with steps at multiples of 0.125 MW (the grain of load - capacity), so the
    target is met on (12.375, 12.5] at least, and the first bracketing pair is the one that holds 12.375: with the bracket (0, 28) and
    two rounds the grid is 12 + k * 4 / 7, whose pair (12, 12.571) holds p as well.  A synthetic solar resource is worth more than
    nothing and less than its largest output."""
    gens, load = small_model
    kw = dict(seed=5, chains=2000, start="stationary", engine=engine)
    p = 12.5
    W = hl1_variable.WeatherYears(np.full((3, 1, 168), p))
    r = hl1_variable.resource_elcc(gens, load, W, [0], 2000, bracket=(0.0, 28.0), rounds=2, **kw)
    base = hl1.run_sequential_mc(gens, load, 2000, **kw)
    assert r.target == base.lole_hours_yr and r.rounds == 2 and r.mode == "shift"
    assert r.pair[0] <= p <= r.pair[1] and r.pair[0] <= r.value <= r.pair[1]
    assert r.pair[1] - r.pair[0] == pytest.approx(28.0 / 7 ** 2, rel=1e-9)
    d = hl1_variable.resource_elcc(gens, load, W, [0], 2000, rounds=1, **kw)              # the default bracket is (0, p): the root is its end
    assert d.pair[1] == p and d.pair[0] <= d.value <= p
    S = hl1_variable.synthetic_weather(3, hours=168, solar_mw=40.0, wind_mw=30.0, seed=3)
    top = float(S.output_mw[:, 0].max())
    for metric in ("lole", "eue"):
        e = hl1_variable.resource_elcc(gens, load, S, [0], 2000, metric=metric, **kw)
        assert 0.0 <= e.pair[0] <= e.value <= e.pair[1] <= top and 0.0 < e.value < top
        assert min(e.pair_metric) <= e.target <= max(e.pair_metric) and 0 < e.std_error < top
    wind_there = hl1_variable.run_sequential_variable(gens, load, S, 2000, resource_scale=(0.0, 1.0), **kw)
    assert e.target == wind_there.eue_mwh_yr                                              # the other resource is there on both sides
