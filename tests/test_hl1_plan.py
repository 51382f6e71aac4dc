"""HL1 planning model on the GPU (relmc_hl1_plan; generating_adequancy_comparative.jl:15-120, tail_risk.jl:12-91): the device against
the host model (tests/tools/hl1_plan_model.py) year for year and hour for hour, split / repeat invariance, the ELU limits, the exact
continuous-normal expectation, the Python surface and the error codes."""
import ctypes as C
import importlib.util
import math
import os

import numpy as np
import pytest

from powersystemsreliabilityassessment_amd import _abi, hl1, hl1_planning as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("hl1_plan_model", os.path.join(ROOT, "tests", "tools", "hl1_plan_model.py"))
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)

dp = _abi.c_double_p


def _load(eng, cap, forr, start, weeks, limit, load, sigma):
    f = [np.ascontiguousarray(x, dtype=np.float64) for x in (cap, forr, limit, load)]
    i = [np.ascontiguousarray(x, dtype=np.int32) for x in (start, weeks)]
    rc = eng.L.relmc_hl1_plan_load(eng._h, f[0].size, f[0].ctypes.data_as(dp), f[1].ctypes.data_as(dp), i[0].ctypes.data_as(_abi.c_int32_p),
                                   i[1].ctypes.data_as(_abi.c_int32_p), f[2].ctypes.data_as(dp), f[3].size, f[3].ctypes.data_as(dp), sigma)
    eng._hl1_plan_loaded = None                    # hl1_planning's cache no longer describes the device
    return rc


def _run(eng, seed, first, n, nhours, n_elu):
    acc = _abi.Hl1SeqAcc()
    yr = np.zeros((n, 3))
    hours = np.zeros(nhours, dtype=np.int64)
    elu = np.zeros((n, max(n_elu, 1)))
    eng._check(eng.L.relmc_hl1_plan(eng._h, seed, first, n, C.byref(acc), yr.ctypes.data_as(C.POINTER(_abi.Hl1SeqYear)),
                                    hours.ctypes.data_as(_abi.c_int64_p), elu.ctypes.data_as(dp)), "relmc_hl1_plan")
    return acc, yr, hours, elu[:, :n_elu]


def _check(eng, data, sigma, seed, first, n):
    assert _load(eng, *data, sigma) == 0
    n_elu = int(np.isfinite(np.asarray(data[4])).sum())
    acc, yr, hours, elu = _run(eng, seed, first, n, len(data[5]), n_elu)
    lole, eue, lolf, counts, energy, ties = M.model(seed, range(first, first + n), *data, sigma)
    assert ties == 0
    np.testing.assert_array_equal(yr[:, 0], lole)
    np.testing.assert_array_equal(yr[:, 2], lolf)
    np.testing.assert_array_equal(hours, counts)
    np.testing.assert_allclose(yr[:, 1], eue, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(elu, energy, rtol=1e-9, atol=1e-9)
    assert acc.years == n and acc.sum_lole == pytest.approx(lole.sum(), rel=1e-12) and acc.sum_lolf == pytest.approx(lolf.sum(), rel=1e-12)
    return yr, hours, elu


def _toy():
    units, load = P.toy_fleet(), P.toy_load(1)
    P.schedule_maintenance(units, P.weekly_peaks(load))
    return [np.array(x) for x in ([u.capacity for u in units], [u.for_rate for u in units], [u.scheduled_outage_start for u in units],
                                  [u.maintenance_weeks for u in units], [u.energy_limit for u in units])] + [load], float(load.max()) * 0.05


def _rts24():
    units, load = P.rts24_planning_units(), hl1.rts24_load().hourly_load
    P.schedule_maintenance(units, P.weekly_peaks(load))
    return [np.array(x) for x in ([u.capacity for u in units], [u.for_rate for u in units], [u.scheduled_outage_start for u in units],
                                  [u.maintenance_weeks for u in units], [u.energy_limit for u in units])] + [load]


@pytest.mark.gpu
def test_device_equals_host_model_toy(engine):
    """Toy fleet, 5 % LFU, binding ELU, scheduled maintenance; years past 2^32 too."""
    data, sigma = _toy()
    yr, hours, elu = _check(engine, data, sigma, 3, 0, 130)
    assert (elu[:, 0] >= 10000.0).all() and yr[:, 0].min() > 0
    _check(engine, data, sigma, 4, (1 << 32) - 20, 64)


@pytest.mark.gpu
def test_device_equals_host_model_rts24(engine):
    data = _rts24()
    yr, hours, _ = _check(engine, data, 0.02 * float(data[5].max()), 9, 1000, 192)
    assert yr[:, 0].sum() > 0


@pytest.mark.gpu
def test_device_equals_host_model_100_units(engine):
    """100 units (past 64: two Philox word groups per lane boundary), 3 ELUs, a 1000-hour year with maintenance."""
    data = M.fleet100()
    yr, hours, elu = _check(engine, data, 100.0, 5, 7, 100)
    lim = data[4][np.isfinite(data[4])]
    assert (elu >= lim).any() and (elu < lim).any() and yr[:, 0].sum() > 100


@pytest.mark.gpu
def test_split_and_repeat_invariance(engine):
    data, sigma = _toy()
    assert _load(engine, *data, sigma) == 0
    N, a = 1500, 611
    acc, yr, hours, elu = _run(engine, 8, 0, N, 8760, 1)
    acc1, yr1, h1, e1 = _run(engine, 8, 0, a, 8760, 1)
    acc2, yr2, h2, e2 = _run(engine, 8, a, N - a, 8760, 1)
    assert np.array_equal(yr, np.vstack([yr1, yr2])) and np.array_equal(elu, np.vstack([e1, e2])) and np.array_equal(hours, h1 + h2)
    for f in ("sum_lole", "sum_eue", "sum_lolf", "sum_lole2", "sum_eue2", "sum_lolf2"):
        assert getattr(acc, f) == pytest.approx(getattr(acc1, f) + getattr(acc2, f), rel=1e-12), f
    r = _run(engine, 8, 0, N, 8760, 1)
    assert np.array_equal(r[1], yr) and np.array_equal(r[2], hours) and np.array_equal(r[3], elu)
    assert (r[0].sum_lole, r[0].sum_eue, r[0].sum_lolf, r[0].sum_eue2) == (acc.sum_lole, acc.sum_eue, acc.sum_lolf, acc.sum_eue2)


@pytest.mark.gpu
def test_absent_units(engine):
    """A unit appended as an ELU with limit 0, or in maintenance all year, gives exactly the results of the fleet without it (its Philox
    word comes last, so the other units' draws do not move)."""
    cap, forr, start, weeks, limit, load = M.fleet100()
    base = [cap, forr, start, weeks, limit, load]
    assert _load(engine, *base, 80.0) == 0
    ref = _run(engine, 2, 0, 96, load.size, 3)
    extra = [np.append(cap, 140.0), np.append(forr, 0.05), np.append(start, 0), np.append(weeks, 0), np.append(limit, 0.0), load]
    assert _load(engine, *extra, 80.0) == 0
    got = _run(engine, 2, 0, 96, load.size, 4)
    assert np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2]) and np.array_equal(got[3][:, :3], ref[3])
    assert not got[3][:, 3].any()
    extra = [np.append(cap, 140.0), np.append(forr, 0.05), np.append(start, 1), np.append(weeks, 6), np.append(limit, math.inf), load]
    assert _load(engine, *extra, 80.0) == 0
    got = _run(engine, 2, 0, 96, load.size, 3)
    assert np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2]) and np.array_equal(got[3], ref[3])


@pytest.mark.gpu
def test_unbounded_elu_is_a_thermal_unit(engine):
    """An ELU whose limit is never reached (1e300 MWh) matches the same unit as a thermal unit: loss counts exact, EUE to 1e-9."""
    data = _rts24()
    sigma = 0.03 * float(data[5].max())
    assert _load(engine, *data, sigma) == 0
    ref = _run(engine, 6, 0, 256, 8736, 0)
    lim = data[4].copy()
    lim[12] = 1e300
    assert _load(engine, data[0], data[1], data[2], data[3], lim, data[5], sigma) == 0
    got = _run(engine, 6, 0, 256, 8736, 1)
    assert np.array_equal(got[1][:, 0], ref[1][:, 0]) and np.array_equal(got[1][:, 2], ref[1][:, 2]) and np.array_equal(got[2], ref[2])
    np.testing.assert_allclose(got[1][:, 1], ref[1][:, 1], rtol=1e-9, atol=1e-9)
    assert ref[1][:, 0].sum() > 0 and got[3].max() > 0


def _exact_normal(data, sigma):
    """sum_h sum_s p_s P(load_h + sigma Z > cap_s) and the expected deficit, from weekly COPTs at step 1 MW (integer capacities)."""
    cap, forr, start, weeks, _, load = data
    units = [P.PlanningUnit(str(k), float(cap[k]), float(forr[k]), int(weeks[k]), scheduled_outage_start=int(start[k])) for k in range(cap.size)]
    erfc = np.frompyfunc(math.erfc, 1, 1)
    lole = eue = 0.0
    for w in range(1, 53):
        h0, h1 = (w - 1) * 168, min(w * 168, load.size)
        week = [u for u in units if not u.in_maintenance(w)]
        probs, installed = P._copt([u.capacity for u in week], [u.for_rate for u in week], 1.0)
        avail = installed - np.arange(probs.size)
        keep = probs > 1e-18
        p, a = probs[keep], avail[keep]
        t = (load[h0:h1, None] - a[None, :]) / sigma                          # P(loss) = Phi(t), E[deficit] = sigma (phi(t) + t Phi(t))
        near = t > -12.0
        Phi = np.zeros_like(t)
        Phi[near] = 0.5 * erfc(-t[near] / math.sqrt(2.0)).astype(np.float64)
        phi = np.exp(-0.5 * t * t) / math.sqrt(2.0 * math.pi)
        lole += float(np.sum(Phi @ p))
        eue += float(np.sum((sigma * (phi + t * Phi)) @ p))
    return lole, eue


@pytest.mark.gpu
def test_rts24_against_the_exact_normal_expectation(engine):
    """ELU-free RTS-24 with its maintenance schedule and 3 % LFU: Monte Carlo LOLE and EUE within 4.5 standard errors of the exact
    continuous-normal expectation (not the 7-step LFU)."""
    data = _rts24()
    sigma = 0.03 * float(data[5].max())
    assert _load(engine, *data, sigma) == 0
    n = 200000
    acc, yr, _, _ = _run(engine, 31, 0, n, 8736, 0)
    el, ee = _exact_normal(data, sigma)
    for s, s2, e in ((acc.sum_lole, acc.sum_lole2, el), (acc.sum_eue, acc.sum_eue2, ee)):
        m = s / n
        se = math.sqrt(max(s2 / n - m * m, 0.0) / n)
        assert abs(m - e) < 4.5 * se, (m, e, se)


@pytest.mark.gpu
def test_python_surface(engine):
    units, load = P.toy_fleet(), P.toy_load(1)
    P.schedule_maintenance(units, P.weekly_peaks(load))
    before = hl1.run_non_sequential_mc(hl1.rts24_generators(), hl1.rts24_load(), 20000, seed=3, engine=engine)
    mc = P.run_monte_carlo_simulation(units, load, 5.0, 2000, seed=2, engine=engine)
    after = hl1.run_non_sequential_mc(hl1.rts24_generators(), hl1.rts24_load(), 20000, seed=3, engine=engine)
    assert (before.lole_hours_yr, before.eue_mwh_yr) == (after.lole_hours_yr, after.eue_mwh_yr)
    assert isinstance(mc, hl1.ReliabilityResult) and mc.elu_names == ["Hydro_ELU"] and mc.elu_energy.shape == (2000, 1)
    assert mc.year_lole.shape == mc.year_eue.shape == mc.year_lolf.shape == (2000,) and len(mc.convergence_history) == 20
    np.testing.assert_array_equal(mc.convergence_history, np.cumsum(mc.year_lole)[99::100] / np.arange(100, 2001, 100))
    assert mc.lole_hours_yr == pytest.approx(mc.year_lole.mean(), rel=1e-12) and mc.lolf_occ_yr == pytest.approx(mc.year_lolf.mean(), rel=1e-12)
    assert mc.hourly_loss_prob.shape == (8760,) and mc.hourly_loss_prob.sum() == pytest.approx(mc.lole_hours_yr, rel=1e-12)
    data, sigma = _toy()
    m = M.model(2, range(3), *data, sigma)
    np.testing.assert_array_equal(mc.year_lole[:3], m[0])
    ana = P.run_detailed_analytical(units, load, 5.0)
    text = P.comparison_report(ana, mc)
    assert ("%.4f" % ana.lole_hours_yr) in text and ("%.4f" % mc.lole_hours_yr) in text
    assert "Monte Carlo (ELU)" in hl1.compare_results([ana, mc])
    s = P.tail_summary(mc.year_lole)
    assert s["quantile"][0.99] >= s["quantile"][0.9] and s["tail_mean"][0.99] >= s["quantile"][0.99]
    again = P.run_monte_carlo_simulation(units, load, 5.0, 2000, seed=2, engine=engine)
    assert np.array_equal(again.year_eue, mc.year_eue) and np.array_equal(again.hourly_loss_prob, mc.hourly_loss_prob)


@pytest.mark.gpu
def test_error_codes(engine):
    L = engine.L
    h = C.c_void_p()
    assert L.relmc_ctx_create(0, C.byref(h)) == 0
    try:
        acc = _abi.Hl1SeqAcc()
        assert L.relmc_hl1_plan(h, 1, 0, 4, C.byref(acc), None, None, None) == -5                     # RELMC_ERR_NO_CASE
        cap, forr, start, weeks, limit, load = M.fleet100()

        def ld(n=cap.size, c=cap, f=forr, s=start, w=weeks, lim=limit, nh=load.size, lo=load, sig=10.0):
            c, f, lim, lo = (None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (c, f, lim, lo))
            s, w = (None if a is None else np.ascontiguousarray(a, dtype=np.int32) for a in (s, w))
            ptr = lambda a, t: None if a is None else a.ctypes.data_as(t)
            return L.relmc_hl1_plan_load(h, n, ptr(c, dp), ptr(f, dp), ptr(s, _abi.c_int32_p), ptr(w, _abi.c_int32_p), ptr(lim, dp),
                                         nh, ptr(lo, dp), sig)
        put = lambda a, i, v: np.where(np.arange(a.size) == i, v, a)
        assert ld(c=None) == -1 and ld(f=None) == -1 and ld(s=None) == -1 and ld(w=None) == -1 and ld(lim=None) == -1 and ld(lo=None) == -1
        assert ld(n=0) == -1 and ld(nh=0) == -1 and ld(nh=1 << 29) == -1
        assert ld(sig=-1.0) == -1 and ld(sig=math.nan) == -1 and ld(sig=math.inf) == -1
        assert ld(s=put(start, 4, -1)) == -1 and ld(w=put(weeks, 9, -2)) == -1
        for v in (math.inf, -math.inf, math.nan):
            assert ld(c=put(cap, 3, v)) == -1, v
        assert ld(lim=put(limit, 7, -1.0)) == -1 and ld(lim=put(limit, 7, math.nan)) == -1
        assert ld(f=put(forr, 2, 1.5)) == -1 and ld(f=put(forr, 2, math.nan)) == -1
        nine = limit.copy()
        nine[10:16] = 500.0                                                                              # 3 + 6 = 9 ELUs
        assert ld(lim=nine) == -4                                                                        # RELMC_ERR_UNSUPPORTED
        big = np.ones(129)
        assert ld(n=129, c=big, f=big * 0.1, s=np.zeros(129), w=np.zeros(129), lim=big * math.inf) == -4
        assert L.relmc_hl1_plan(h, 1, 0, 4, C.byref(acc), None, None, None) == -5                     # nothing loaded yet
        assert ld() == 0
        assert L.relmc_hl1_plan(h, 1, 0, 4, None, None, None, None) == -1
        assert L.relmc_hl1_plan(h, 1, 0, -1, C.byref(acc), None, None, None) == -1
        assert L.relmc_hl1_plan(None, 1, 0, 4, C.byref(acc), None, None, None) == -1
        hours = np.full(load.size, 7, dtype=np.int64)
        assert L.relmc_hl1_plan(h, 1, 0, 0, C.byref(acc), None, hours.ctypes.data_as(_abi.c_int64_p), None) == 0
        assert acc.years == 0 and not hours.any()
        assert L.relmc_hl1_plan(h, 1, 0, 8, C.byref(acc), None, None, None) == 0 and acc.years == 8
        # the planning model leaves the other HL1 models alone: none was loaded on this context
        assert L.relmc_hl1_seq(h, 1, 0, 4, 1, 0, C.byref(acc), None) == -5
    finally:
        L.relmc_ctx_destroy(h)
