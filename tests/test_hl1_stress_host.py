"""Weather-dependent forced outage rates on the HL1 sequential chronology (relmc_hl1_stress_seq) without a GPU: the library's two host
functions against the host model bit for bit, on random draws and at the contract's edges; the contract's five consequences on the
model; the model against a plain hour loop and against the exact recursion of a unit's DOWN probability; the analytical counterpart;
the C ABI's exports and the Python argument checks that need no device.  The library's own refusals need a context, which needs a
device: they are in tests/test_hl1_stress.py."""
import ctypes as C
import importlib.util
import math
import os
import re

import numpy as np
import pytest

from powersystemsreliabilityassessment_amd import _abi, _lib, hl1, hl1_storage, hl1_stress, hl1_variable

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("hl1_stress_model", os.path.join(ROOT, "tests", "tools", "hl1_stress_model.py"))
XM = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(XM)
VM, SM, M = XM.VM, XM.SM, XM.SEQ

dp, ip = _abi.c_double_p, _abi.c_int32_p
H = 200
SYMS = ("relmc_hl1_stress_load", "relmc_hl1_stress_seq", "relmc_hl1_stress_cumulative", "relmc_hl1_stress_failure_time")
SMALL_STORAGES = [(20.0, 20.0, 60.0, 0.9, 0.95, 60.0), (10.0, 15.0, 30.0, 0.85, 1.0, 0.0)]


def _lib_time(T, E, nh, years, weather, cum):
    """relmc_hl1_stress_failure_time; cum[n_weather, nh + 1] of one class."""
    w = np.ascontiguousarray(weather, dtype=np.int32)
    g = np.ascontiguousarray(cum, dtype=np.float64)
    return _lib.load().relmc_hl1_stress_failure_time(float(T), float(E), nh, years, w.ctypes.data_as(ip), g.ctypes.data_as(dp))


def _both(T, E, years, weather, cum):
    """The failure time from the library and from the model, which must be the same double."""
    a = _lib_time(T, E, cum.shape[1] - 1, years, weather, cum)
    b = XM.failure_time(T, E, cum.shape[1] - 1, years, [int(v) for v in weather], [r.tolist() for r in cum])
    assert a == b, (T, E, weather, a, b)
    return b


def _small(nh=H):
    cap, mttf, mttr, load = M.small_fleet()
    return cap, mttf, mttr, np.resize(load, nh)


def test_library_exports_the_stress_entry_points():
    hdr = open(os.path.join(ROOT, "include", "relmc.h")).read()
    jl = open(os.path.join(ROOT, "julia", "RelMC.jl")).read()
    mk = open(os.path.join(ROOT, "powersystemsreliabilityassessment_amd", "csrc", "Makefile")).read()
    for sym in SYMS:
        assert re.search(r"\b%s\s*\(" % sym, hdr) and sym in _lib.EXPORTS and (":" + sym) in jl, sym
    assert re.search(r"#define RELMC_HL1_STRESS_MAX_CLASSES\s+%d\b" % _abi.HL1_STRESS_MAX_CLASSES, hdr) and "HL1_STRESS_MAX_CLASSES = 8" in jl
    assert re.search(r"^UNITS = .*\brelmc_stress\b", mk, re.M) and re.search(r"^HDRS = .*\brelmc_hl1_storage_kernels\.h\b", mk, re.M)
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = _lib.load()
    assert all(hasattr(L, s) for s in SYMS)
    assert L.relmc_hl1_stress_seq.argtypes == L.relmc_hl1_var_seq.argtypes and L.relmc_hl1_stress_failure_time.restype is C.c_double


def test_cumulative_equals_the_model():
    L = _lib.load()
    rng = np.random.default_rng(3)
    for row in (XM.edge_multipliers(H)[0, 0], XM.varying_multipliers(1, 1, 1000, 5)[0, 0], rng.uniform(0.0, 1e6, 37), np.zeros(5), np.array([0.1])):
        row = np.ascontiguousarray(row)
        out = np.full(row.size + 1, -1.0)
        assert L.relmc_hl1_stress_cumulative(row.size, row.ctypes.data_as(dp), out.ctypes.data_as(dp)) == 0
        assert out.tobytes() == XM.cumulative(row).tobytes() and out[0] == 0.0
    out = np.full(4, -1.0)
    for bad in ([1.0, float("nan"), 1.0], [1.0, -0.5, 1.0], [float("inf"), 0.0, 0.0]):
        assert L.relmc_hl1_stress_cumulative(3, np.array(bad).ctypes.data_as(dp), out.ctypes.data_as(dp)) == -1 and np.all(out == -1.0)
    assert L.relmc_hl1_stress_cumulative(0, out.ctypes.data_as(dp), out.ctypes.data_as(dp)) == -1
    assert L.relmc_hl1_stress_cumulative(3, None, out.ctypes.data_as(dp)) == -1


def test_failure_time_equals_the_model_on_random_draws():
    """4000 draws on the edge library (zero stretches, a zero year, a spike) and 2000 on a library whose every addition rounds."""
    rng = np.random.default_rng(11)
    never = 0
    for mult, nh, n in ((XM.edge_multipliers(H)[:, 0], H, 4000), (XM.varying_multipliers(3, 1, 1000, 9)[:, 0], 1000, 2000)):
        cum = np.array([XM.cumulative(r) for r in mult])
        for _ in range(n):
            years = int(rng.integers(1, 5))
            wy = rng.integers(0, 3, years)
            T = float(rng.uniform(0.0, years * nh)) if rng.uniform() < 0.9 else float(rng.integers(0, years * nh))
            E = float(-400.0 * math.log(rng.uniform()) * rng.choice([0.003, 0.3, 1.0, 3.0]))
            r = _both(T, E, years, wy, cum)
            assert r >= T
            never += r == years * nh + 1
    assert 500 < never < 5000


def test_failure_time_at_the_edges():
    m = XM.edge_multipliers(H)[:, 0]                               # w 0: zero stretches, w 1: all zero, w 2: a spike of 50 at hour H // 3
    cum = np.array([XM.cumulative(r) for r in m])
    g0, g2 = cum[0], cum[2]
    # a zero stretch at the start of the year: nothing is spent in it, the unit fails in the first hour with a multiplier
    r = _both(3.25, 0.125 * m[0, 17], 1, [0], cum)
    assert r == 17.125
    # in the middle: UP inside the stretch, the draw ends behind it; and a draw that ends exactly at its first edge stays before it
    j1 = H // 2 + 12
    assert _both(H // 2 + 0.5, 0.5 * m[0, j1], 1, [0], cum) == j1 + 0.5
    j0 = H // 2 - 9
    assert _both(float(j0 - 1), m[0, j0 - 1], 1, [0], cum) == float(j0)
    # at the end: what is left of the draw goes to the next year (w 2), whose first hour takes it
    left = g0[H] - g0[H - 30]
    r = _both(float(H - 30), left + 0.25 * m[2, 0], 2, [0, 2], cum)
    assert r == H + 0.25
    # a whole zero year is passed with the draw unchanged (consequence 4): the time in year 2 is the time in a chain that starts there
    E = 7.3
    one = _both(0.0, E, 1, [2], cum)
    two = _both(0.0, E, 3, [1, 1, 2], cum)
    assert one < H and two == pytest.approx(2 * H + one, rel=1e-15) and math.floor(two) == 2 * H + math.floor(one)
    assert _both(5.5, 1e-300, 2, [1, 1], cum) == 2 * H + 1       # nothing but zero years: the unit cannot fail
    # E == rem exactly: not strictly greater, so the unit fails in this year, at the end of its last hour with a multiplier
    T = 40.75
    a = g0[40] + (g0[41] - g0[40]) * 0.75
    rem = g0[H] - a
    r = _both(T, rem, 2, [0, 2], cum)
    assert H - 24 <= r <= H - 23 + 1e-9
    assert _both(T, math.nextafter(rem, math.inf), 2, [0, 2], cum) >= H
    # a draw that outlasts the chain
    assert _both(10.0, 1e9, 3, [0, 2, 0], cum) == 3 * H + 1
    assert _both(10.0, g0[H] - g0[10] + g2[H] + 1.0, 2, [0, 2], cum) == 2 * H + 1
    # the spike: several sojourns end inside one hour, each later than the one before
    js = H // 3
    t, seen = js + 0.01, []
    for _ in range(6):
        t = _both(t, 2.0, 1, [2], cum)
        seen.append(t)
        t = t + 0.02                                               # a short repair
    assert all(js < v < js + 1 for v in seen) and seen == sorted(seen) and len(set(seen)) == 6
    # T exactly on a year boundary belongs to the new year; at or beyond the chain's end there is nothing to see
    assert _both(float(H), 0.5 * m[2, 0], 2, [1, 2], cum) == H + 0.5
    assert _both(float(H), 1.0, 2, [2, 1], cum) == 2 * H + 1
    assert _both(float(2 * H), 1.0, 2, [2, 2], cum) == 2 * H + 1 and _both(2.0 * H + 7.5, 1.0, 2, [2, 2], cum) == 2 * H + 7.5
    # the library refuses what is out of its rules
    bad = [(-1.0, 1.0, H, 1, [0]), (float("nan"), 1.0, H, 1, [0]), (1.0, -1.0, H, 1, [0]), (1.0, 1.0, 0, 1, [0]), (1.0, 1.0, H, 0, [0]),
           (1.0, 1.0, H, 1, [-1]), (1.0, 1.0, H, 1, [256])]
    for T, E, nh, years, wy in bad:
        assert math.isnan(_lib_time(T, E, nh, years, wy, cum))


@pytest.mark.parametrize("start", [M.ALL_UP, M.STATIONARY])
@pytest.mark.parametrize("pick", [VM.PICK_RANDOM, VM.PICK_CYCLE])
def test_consequence_1_class_minus_one_is_the_variable_model(start, pick):
    cap, mttf, mttr, load = _small()
    rng = np.random.default_rng(5)
    out = np.round(rng.uniform(0.0, 20.0, (3, 2, H)), 2)
    kw = dict(resource_scale=[1.0, 0.5], pick=pick, storages=SMALL_STORAGES, shift=3.0)
    rec, wy = XM.stress_model(7, range(6), cap, mttf, mttr, load, 3, start, out, XM.edge_multipliers(H), [-1] * 6, **kw)
    want, wy0 = VM.variable_model(7, range(6), cap, mttf, mttr, load, 3, start, out, **kw)
    assert rec.tobytes() == want.tobytes() and np.array_equal(wy, wy0) and rec[:, 0].sum() > 0 and rec[:, 3].sum() > 0


def test_consequence_2_constant_multipliers_in_one_year_chains():
    """Multiplier 1.0: the variable model bit for bit; exactly 2.0 for one class: the variable model with those units' mttf halved."""
    cap, mttf, mttr, load = _small()
    out = np.zeros((3, 0, H))
    cnt = {}
    one = np.ones((3, 2, H))
    rec, _ = XM.stress_model(7, range(300), cap, mttf, mttr, load, 1, M.ALL_UP, out, one, [0, 1, 0, 1, 0, 1], counters=cnt)
    want, _ = VM.variable_model(7, range(300), cap, mttf, mttr, load, 1, M.ALL_UP, out)
    assert rec.tobytes() == want.tobytes() and cnt["failures"] > 2000 and 0 < cnt["never"] < cnt["failures"]
    two = one.copy()
    two[:, 1, :] = 2.0
    rec, _ = XM.stress_model(7, range(300), cap, mttf, mttr, load, 1, M.ALL_UP, out, two, [-1, 1, 0, 1, 0, 1])
    half = mttf.copy()
    half[[1, 3, 5]] /= 2.0
    want2, _ = VM.variable_model(7, range(300), cap, half, mttr, load, 1, M.ALL_UP, out)
    assert rec.tobytes() == want2.tobytes() and rec.tobytes() != want.tobytes() and rec[:, 0].sum() > want[:, 0].sum()


def test_consequence_3_multiplier_one_in_long_chains():
    """No bitwise guarantee: the transition times may differ in the last bit.  On these chains some do, and no step changes."""
    cap, mttf, mttr, load = _small()
    out = np.zeros((3, 0, H))
    one = np.ones((3, 1, H))
    rec, _ = XM.stress_model(7, range(40), cap, mttf, mttr, load, 5, M.STATIONARY, out, one, [0] * 6)
    want, _ = VM.variable_model(7, range(40), cap, mttf, mttr, load, 5, M.STATIONARY, out)
    np.testing.assert_array_equal(rec[:, [0, 2, 3]], want[:, [0, 2, 3]])
    np.testing.assert_allclose(rec[:, 1], want[:, 1], rtol=1e-12)
    W = VM.weather_years(7, range(40), 5, 3, VM.PICK_RANDOM)
    _, T = XM.stress_chronology(7, range(40), mttf, mttr, M.STATIONARY, H, 5, W, XM.cumulative_tables(one), [0] * 6)
    _, T0, _ = M.chronology(7, np.arange(40, dtype=np.uint64), mttf, mttr, M.STATIONARY, 5 * H)
    n = min(T.shape[2], T0.shape[2])
    seen = (T[:, :, :n] < 5 * H) & (T0[:, :, :n] < 5 * H)
    a, b = T[:, :, :n][seen], T0[:, :, :n][seen]
    assert a.size > 1000 and np.any(a != b) and np.all(np.abs(a - b) <= 1e-13 * b)


def test_consequence_5_class_minus_one_units_keep_their_history():
    cap, mttf, mttr, load = _small()
    cls = [0, -1, 1, -1, 0, -1]
    W = VM.weather_years(7, range(12), 3, 3, VM.PICK_RANDOM)
    for start in (M.ALL_UP, M.STATIONARY):
        d, T = XM.stress_chronology(7, range(12), mttf, mttr, start, H, 3, W, XM.cumulative_tables(XM.edge_multipliers(H)), cls)
        d0, T0, _ = M.chronology(7, np.arange(12, dtype=np.uint64), mttf, mttr, start, 3 * H)
        assert np.array_equal(d, d0)
        differ = 0
        for k, c in enumerate(cls):
            for ch in range(12):
                n = int(np.searchsorted(T0[ch, k], 3 * H, side="right")) + 1          # the times within the chain and the first beyond
                if c < 0:
                    assert T[ch, k, :n].tobytes() == T0[ch, k, :n].tobytes()
                else:
                    differ += T[ch, k, :n].tobytes() != T0[ch, k, :n].tobytes()
        assert differ > 12


@pytest.mark.parametrize("start", [M.ALL_UP, M.STATIONARY])
def test_model_against_the_plain_hour_loop(start):
    """The hour loop works on the multipliers, the model on the cumulative table, so their times differ in the last bits; the loss hours and
    the events of every year are the same on these chains, the energies to rounding."""
    cap, mttf, mttr, load = _small()
    rng = np.random.default_rng(5)
    out = np.round(rng.uniform(0.0, 20.0, (3, 1, H)), 2)
    cls = [0, 0, 1, 0, -1, 1]
    for mult in (XM.edge_multipliers(H), XM.varying_multipliers(3, 2, H, 4)):
        total = 0.0
        for c in (0, 3, 5, 8):
            kw = dict(resource_scale=[0.5], pick=VM.PICK_CYCLE, shift=-4.0)
            rec, wy = XM.stress_model(7, [c], cap, mttf, mttr, load, 3, start, out, mult, cls, **kw)
            lit, lw = XM.literal_stress_chain(7, c, cap, mttf, mttr, load, 3, start, out, mult, cls, **kw)
            np.testing.assert_array_equal(rec[:, [0, 2]], lit[:, [0, 2]])
            np.testing.assert_allclose(rec[:, 1], lit[:, 1], rtol=1e-12)
            assert np.array_equal(wy, lw)
            total += rec[:, 0].sum()
        assert total > 0


def test_sampled_down_probability_against_the_recursion():
    """One unit, H = 120, started UP, 20000 one-year chains of the model: the share of chains in which it is DOWN at step n lies within
    4.5 standard errors (of the exact probability) of hourly_down_probability at every step."""
    nh, n = 120, 20000
    mult = XM.varying_multipliers(1, 1, nh, 21)
    mult[0, 0, 30:40] = 0.0
    mult[0, 0, 70] = 25.0
    mttf, mttr = [60.0], [15.0]
    want = XM.hourly_down_probability(mult[0, 0], mttf[0], mttr[0])
    d0, T = XM.stress_chronology(5, range(n), mttf, mttr, M.ALL_UP, nh, 1, np.zeros((n, 1), dtype=np.int64), XM.cumulative_tables(mult), [0])
    steps = np.arange(1, nh + 1, dtype=np.float64)
    down = np.zeros(nh)
    for c in range(n):
        down += np.searchsorted(T[c, 0], steps, side="right") & 1
    se = np.sqrt(want * (1.0 - want) / n)
    z = (down / n - want) / se
    print("max |z| over the hours: %.2f" % np.abs(z).max())
    assert not d0.any() and np.abs(z).max() < 4.5
    flat = XM.hourly_down_probability(np.ones(nh), mttf[0], mttr[0])
    assert np.abs((down / n - flat) / se).max() > 10.0             # the constant-rate unit is far away: the multipliers are felt
    q, rate = mttr[0] / (mttf[0] + mttr[0]), 1.0 / mttf[0] + 1.0 / mttr[0]
    np.testing.assert_allclose(flat, q * (1.0 - np.exp(-rate * steps)), rtol=1e-12)


def _gens(cap, mttf, mttr):
    return [hl1.Generator(i + 1, float(cap[i]), float(mttf[i]), float(mttr[i])) for i in range(len(cap))]


def test_analytical_stress():
    """Multiplier 1: the exact first year of a chain started all UP (hl1_seq_model.all_up_year1, which tests/test_hl1_seq_host.py uses).
    Class -1 is multiplier 1.  Resources enter as a lower net load; a multiplier above 1 in the loaded hours raises both indices."""
    cap, mttf, mttr, load = M.small_fleet()
    gens, ld = _gens(cap, mttf, mttr), hl1.LoadModel(load)
    W0 = hl1_variable.WeatherYears(np.zeros((2, 0, 168)))
    want = M.all_up_year1(cap.astype(int), mttf, mttr, load)
    for stress in (hl1_stress.OutageStress(np.ones((2, 2, 168)), [0, 1, 0, 1, 0, 1]), hl1_stress.OutageStress(np.full((2, 1, 168), 7.0), [-1] * 6)):
        got = hl1_stress.run_analytical_stress(gens, ld, W0, stress)
        assert got.lole_hours_yr == pytest.approx(want[0], rel=1e-10) and got.eue_mwh_yr == pytest.approx(want[1], rel=1e-10)
        assert got.hourly_loss_probability.shape == (168,) and got.hourly_loss_probability.sum() == pytest.approx(got.lole_hours_yr, rel=1e-12)
    rng = np.random.default_rng(2)
    out = np.round(rng.uniform(0.0, 20.0, (2, 1, 168)), 2)
    wl = np.round(load[None, :] * np.array([[0.97], [1.05]]), 2)
    W = hl1_variable.WeatherYears(out, wl)
    one = hl1_stress.OutageStress(np.ones((2, 1, 168)), [0] * 6)
    got = hl1_stress.run_analytical_stress(gens, ld, W, one, resource_scale=[0.5])
    ref = np.mean([M.all_up_year1(cap.astype(int), mttf, mttr, wl[w] - 0.5 * out[w, 0]) for w in range(2)], axis=0)
    assert got.lole_hours_yr == pytest.approx(ref[0], rel=1e-10) and got.eue_mwh_yr == pytest.approx(ref[1], rel=1e-10)
    syn = hl1_stress.synthetic_stress(W, ld, gens)
    hot = hl1_stress.run_analytical_stress(gens, ld, W, syn, resource_scale=[0.5])
    assert hot.lole_hours_yr != got.lole_hours_yr and hot.eue_mwh_yr > 0
    # one unit, one hour-varying multiplier: the hourly table is the recursion itself
    mult = XM.varying_multipliers(1, 1, 168, 3)
    g1 = [hl1.Generator(1, 100.0, 80.0, 20.0)]
    r = hl1_stress.run_analytical_stress(g1, hl1.LoadModel(np.full(168, 50.0)), hl1_variable.WeatherYears(np.zeros((1, 0, 168))),
                                         hl1_stress.OutageStress(mult, [0]))
    np.testing.assert_allclose(r.hourly_loss_probability, XM.hourly_down_probability(mult[0, 0], 80.0, 20.0), rtol=1e-12)
    assert r.eue_mwh_yr == pytest.approx(50.0 * r.lole_hours_yr, rel=1e-12)


def test_synthetic_stress():
    cap, mttf, mttr, load = M.small_fleet()
    gens, ld = _gens(cap, mttf, mttr), hl1.LoadModel(load)
    W = hl1_variable.synthetic_weather(4, hours=168, solar_mw=10.0, wind_mw=10.0, seed=3, load=ld)
    s = hl1_stress.synthetic_stress(W, ld, gens)
    assert s.fail_mult.shape == (4, 2, 168) and s.names == ("large thermal", "small thermal") and s.fail_mult.min() > 0.0
    np.testing.assert_allclose(s.fail_mult.mean(axis=(0, 2)), 1.0, rtol=1e-12)
    assert s.unit_class.tolist() == [0, 0, 0, 0, 1, 1] and s.unit_class.dtype == np.int32
    w, h = np.unravel_index(np.argmax(W.load_mw), W.load_mw.shape)
    assert s.fail_mult[w, 0, h] == s.fail_mult[:, 0].max() > 2.0 and s.fail_mult[w, 0, h] > s.fail_mult[w, 1, h] > 1.0
    for c in range(2):                                             # the multipliers rise with the load of the same weather year and hour
        order = np.argsort(W.load_mw.reshape(-1))
        assert np.all(np.diff(s.fail_mult[:, c].reshape(-1)[order]) >= 0.0)
    one = hl1_stress.synthetic_stress(hl1_variable.WeatherYears(np.zeros((2, 0, 168))), ld, gens, sensitivity=(3.0,), names=("thermal",))
    assert one.fail_mult.shape == (2, 1, 168) and not one.unit_class.any() and np.array_equal(one.fail_mult[0], one.fail_mult[1])
    for kw in (dict(sensitivity=()), dict(sensitivity=(1.0, 2.0, 3.0)), dict(sensitivity=(-1.0,)), dict(threshold=1.0)):
        with pytest.raises(ValueError):
            hl1_stress.synthetic_stress(W, ld, gens, **kw)
    with pytest.raises(ValueError):
        hl1_stress.synthetic_stress(W, ld, [])


class _Untouchable:
    """Stands in for the engine: any use of it fails the test."""
    def __getattr__(self, name):
        raise AssertionError(f"the engine was touched ({name}) before the arguments were checked")


def test_stress_arguments_are_checked_before_the_engine():
    cap, mttf, mttr, load = M.small_fleet()
    gens, ld = _gens(cap, mttf, mttr), hl1.LoadModel(load)
    rng = np.random.default_rng(5)
    W = hl1_variable.WeatherYears(np.round(rng.uniform(0.0, 20.0, (3, 2, 168)), 2))
    mult = XM.edge_multipliers(168)
    cls = [0, 0, 1, 0, -1, 1]
    X = hl1_stress.OutageStress
    ok = X(mult, cls, ("a", "b"))
    nan, inf = float("nan"), float("inf")
    S = hl1_storage.Storage

    def spoiled(idx, v):
        b = mult.copy(); b[idx] = v
        return b

    bad = [dict(years=10, chains=3), dict(years=0), dict(years=10, start="cold"), dict(years=10, scale=nan), dict(years=10, shift=inf),
           dict(years=10, pick="first"), dict(years=10, resource_scale=[1.0]), dict(years=10, resource_scale=[1.0, -0.5]),
           dict(years=10, storages=[S(1.0, 1.0, 1.0)] * 9), dict(years=10, storages=[S(1.0, 1.0, 1.0, eta_charge=0.0)]),
           dict(years=10, weather=hl1_variable.WeatherYears(np.zeros((3, 9, 168)))),
           dict(years=10, stress=X(spoiled((1, 0, 5), -1.0), cls)), dict(years=10, stress=X(spoiled((2, 1, 7), nan), cls)),
           dict(years=10, stress=X(spoiled((0, 0, 0), inf), cls)), dict(years=10, stress=X(mult, [0, 0, 1, 0, -1, 2])),
           dict(years=10, stress=X(mult, [0, 0, 1, 0, -2, 1])), dict(years=10, stress=X(mult, cls[:5])), dict(years=10, stress=X(mult, cls + [0])),
           dict(years=10, stress=X(mult[:2], cls)), dict(years=10, stress=X(mult[:, :, :100], cls)), dict(years=10, stress=X(mult, cls, ("a",))),
           dict(years=10, stress=X(np.ones((3, 9, 168)), cls)), dict(years=10, stress=X(np.ones((3, 0, 168)), [-1] * 6)),
           dict(years=10, stress=X(np.ones((3, 1, 168)), np.zeros(129, dtype=np.int32)))]
    for kw in bad:
        with pytest.raises(ValueError):
            hl1_stress.run_sequential_stress(gens, ld, **{"weather": W, "stress": ok, "engine": _Untouchable(), **kw})
    with pytest.raises(ValueError, match="weather year 2, class 1, hour 7 is not finite"):
        hl1_stress.run_sequential_stress(gens, ld, W, X(spoiled((2, 1, 7), nan), cls), 10, engine=_Untouchable())
    with pytest.raises(ValueError, match="weather year 1, class 0, hour 5 is negative"):
        hl1_stress.run_sequential_stress(gens, ld, W, X(spoiled((1, 0, 5), -1.0), cls), 10, engine=_Untouchable())
    with pytest.raises(ValueError, match="class 2 of unit 5 not in -1..1"):
        hl1_stress.run_sequential_stress(gens, ld, W, X(mult, [0, 0, 1, 0, -1, 2]), 10, engine=_Untouchable())
    with pytest.raises(ValueError, match="5 units, the fleet 6"):
        hl1_stress.run_analytical_stress(gens, ld, W, X(mult, cls[:5]))
    with pytest.raises(ValueError, match="2 weather years, the weather library 3"):
        hl1_stress.run_analytical_stress(gens, ld, W, X(mult[:2], cls))
    with pytest.raises(ValueError, match="100 hours, the weather library 168"):
        hl1_stress.run_analytical_stress(gens, ld, W, X(mult[:, :, :100], cls))
    with pytest.raises(ValueError):
        hl1_stress.run_analytical_stress(gens, ld, W, ok, step_size=0.0)
    with pytest.raises(ValueError):
        hl1_stress.run_analytical_stress(gens, ld, W, ok, resource_scale=[1.0])
    with pytest.raises(ValueError, match="fail_mult must be"):
        X(np.ones((3, 168)), cls)
    with pytest.raises(ValueError, match="unit_class must be"):
        X(mult, [0.5] * 6)
    with pytest.raises(ValueError, match="unit_class must be"):
        X(mult, [[0, 1, 0], [1, 0, 1]])


def test_stress_report():
    base = hl1_variable.VariableReliabilityResult("Sequential MC + resources", 8.0, 1000.0, 0.1, lolf_occ_yr=2.0)
    r = hl1_stress.StressReliabilityResult("Sequential MC + stress", 12.0, 1750.0, 0.1, lolf_occ_yr=2.5,
                                           year_weather=np.array([0, 2, 2, 1], dtype=np.int32), pick="cycle",
                                           unit_class=np.array([0, 1, -1, 0], dtype=np.int32), mean_multiplier=np.array([1.25, 0.875]))
    txt = hl1_stress.stress_report(base, r)
    assert "OUTAGE STRESS SUMMARY" in txt and "8.0000" in txt and "12.0000" in txt and "1750.00" in txt
    assert "3 of 4 units in 2 outage classes over 3 weather years drawn (cycle); mean multiplier per class: 1.250, 0.875" in txt
    assert "LOLE x 1.500, EUE x 1.750 against independent outages" in txt
