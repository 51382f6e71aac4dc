"""Loss attribution on the HL1 sequential chronology on the GPU (relmc_hl1_attr_seq): the year records against relmc_hl1_seq and the sweep
bit for bit, the chains' unit records against the host model (tests/tools/hl1_attr_model.py) bit for bit, the counterfactual identity
against the sweep's withheld fleet exactly in integers, split / repeat / launch invariance, the exact expectations of
run_analytical_attribution, the error codes and the Python layer on RTS-24."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from powersystemsreliabilityassessment_amd import _abi, hl1, hl1_attribution as ha

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("hl1_attr_model", os.path.join(ROOT, "tests", "tools", "hl1_attr_model.py"))
AM = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(AM)
M = AM.SEQ

dp = _abi.c_double_p
YP = C.POINTER(_abi.Hl1SeqYear)
UP = C.POINTER(_abi.Hl1AttrUnit)
ACC_FIELDS = [f for f, _ in _abi.Hl1SeqAcc._fields_]


def _fleet(name):
    return M.small_fleet() if name == "small" else M.fleet100(int(name))


def _cut(n):
    """The first n units of fleet100(513), the load scaled to their share of the capacity."""
    cap, mttf, mttr, load = M.fleet100(513)
    return cap[:n], mttf[:n], mttr[:n], load * (cap[:n].sum() / cap.sum())


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


def _sweep_level(eng, seed, first, n, years, start, scale, shift, fleet, withheld=()):
    arr = (_abi.Hl1SweepLevel * 1)(_abi.Hl1SweepLevel(scale, shift, fleet, 0))
    mask = (C.c_uint32 * 4)()
    for k in withheld:
        mask[k >> 5] |= 1 << (k & 31)
    acc = (_abi.Hl1SeqAcc * 1)()
    yr = np.zeros((n * years, 3))
    eng._check(eng.L.relmc_hl1_seq_sweep(eng._h, seed, first, n, years, start, 1, arr, mask, acc, yr.ctypes.data_as(YP)), "relmc_hl1_seq_sweep")
    return acc[0], yr


def _attr(eng, K, seed, first, n, years, start, scale=1.0, shift=0.0, want_host=True):
    """-> (acc, yr[n * years, 3], unit_acc as (sum[K, 4], sum2[K, 4]), unit_host[n, K, 4])."""
    acc = _abi.Hl1SeqAcc()
    uacc = (_abi.Hl1AttrAcc * K)()
    yr = np.zeros((n * years, 3))
    rec = np.zeros((n, K, 4))
    eng._check(eng.L.relmc_hl1_attr_seq(eng._h, seed, first, n, years, start, scale, shift, C.byref(acc), yr.ctypes.data_as(YP) if want_host else None,
                                        uacc, rec.ctypes.data_as(UP) if want_host else None), "relmc_hl1_attr_seq")
    return acc, yr, (np.array([list(a.sum) for a in uacc]), np.array([list(a.sum2) for a in uacc])), rec


def _acc_tuple(a):
    return tuple(getattr(a, f) for f in ACC_FIELDS)


@pytest.mark.gpu
@pytest.mark.parametrize("start", [M.ALL_UP, M.STATIONARY])
@pytest.mark.parametrize("fleet,n,years,scale,shift", [("513", 16, 5, 1.07, 33.25), ("small", 21, 6, 0.97, 6.5)])
def test_year_records_are_the_sequential_and_the_sweep_kernels_bitwise(engine, fleet, n, years, scale, shift, start):
    cap, mttf, mttr, load = _fleet(fleet)
    _load(engine, cap, mttf, mttr, load)
    a0, ref = _seq(engine, 11, 2, n, years, start)
    a1, lvl = _sweep_level(engine, 11, 2, n, years, start, 1.0, 0.0, 0)
    a2, lvl2 = _sweep_level(engine, 11, 2, n, years, start, scale, shift, 0)
    assert ref[:, 0].sum() > 0 and lvl2[:, 0].sum() != ref[:, 0].sum()
    acc, yr, _, _ = _attr(engine, cap.size, 11, 2, n, years, start)
    assert yr.tobytes() == ref.tobytes() == lvl.tobytes()
    assert _acc_tuple(acc) == _acc_tuple(a0) == _acc_tuple(a1)
    acc, yr, _, _ = _attr(engine, cap.size, 11, 2, n, years, start, scale, shift)
    assert yr.tobytes() == lvl2.tobytes() and _acc_tuple(acc) == _acc_tuple(a2)


def _cases():
    small = M.small_fleet()
    zero_cap = (np.where(np.arange(6) == 2, 0.0, small[0]),) + small[1:]
    return {
        # both lane slots, all four mask words, the window boundary at step 512, a chain count that is no multiple of 4
        "fleet100": (M.fleet100(513), 5, 3, 1.0, 0.0, 2),
        "fleet100-scaled": (M.fleet100(513), 5, 3, 1.03, -4.75, 7),
        "small": (small, 7, 4, 1.0, 0.0, 0),
        "one-unit": (_cut(1), 5, 3, 1.0, 0.0, 1),
        "64-units": (_cut(64), 5, 3, 1.0, 0.0, 1),
        "65-units": (_cut(65), 5, 3, 1.0, 0.0, 1),
        # 4 * 168 = 512 + 160 steps: the chain's last step is lane 31 of its group
        "load-above-the-fleet": (small, 7, 4, 1.0, 1.0e6, 3),
        "load-below-zero": (small, 7, 4, 1.0, -1.0e6, 3),
        "zero-capacity-unit": (zero_cap, 7, 4, 1.0, 0.0, 0),
    }


@pytest.mark.gpu
@pytest.mark.parametrize("start", [M.ALL_UP, M.STATIONARY])
@pytest.mark.parametrize("name", list(_cases()))
def test_unit_records_against_the_host_model_bitwise(engine, name, start):
    (cap, mttf, mttr, load), n, years, scale, shift, first = _cases()[name]
    _load(engine, cap, mttf, mttr, load)
    _, yr, _, rec = _attr(engine, cap.size, 17, first, n, years, start, scale, shift)
    yrs, units = AM.attr_model(17, range(first, first + n), cap, mttf, mttr, load, years, start, scale, shift)
    np.testing.assert_array_equal(yr[:, 0], yrs[0])
    np.testing.assert_array_equal(yr[:, 2], yrs[2])
    for q, f in enumerate(ha.FIELDS):
        np.testing.assert_array_equal(rec[:, :, q], units[:, :, q], err_msg=f)
    assert rec.tobytes() == units.tobytes()
    steps = years * load.size
    if name == "load-above-the-fleet":
        assert np.all(yr[:, 0] == load.size) and np.all(rec[:, :, 2] == 0) and rec[:, :, 0].sum() > 0 and np.all(rec[:, :, 0] <= steps)
    elif name == "load-below-zero":
        assert not rec.any() and not yr.any()
    elif name == "zero-capacity-unit":
        assert rec[:, 2, 0].sum() > 0 and not rec[:, 2, 2].any() and not rec[:, 2, 3].any()
    else:
        assert rec[:, :, 0].sum() > 0 and rec[:, :, 2].sum() > 0


@pytest.mark.gpu
def test_counterfactual_identity_is_exact_in_integers(engine):
    """Integer capacities and loads: every sum is exact.  For every unit k, critical_hours_k and relief_mwh_k summed over the chains are
    the base run's loss hours and EUE minus those of the fleet without k against the load lowered by cap_k (the sweep's fleet 1 with k
    withheld at shift -cap_k): the history with k always UP.  Ties cap_avail + cap_k == L occur with k DOWN, and count as critical."""
    cap, mttf, mttr, load = M.small_fleet()
    load = np.round(load)
    _load(engine, cap, mttf, mttr, load)
    n, years = 64, 6
    acc, yr, (s1, _), rec = _attr(engine, cap.size, 5, 0, n, years, M.STATIONARY)
    assert acc.sum_lole == yr[:, 0].sum() > 0 and acc.sum_eue == yr[:, 1].sum()
    for k in range(cap.size):
        a, _ = _sweep_level(engine, 5, 0, n, years, M.STATIONARY, 1.0, -float(cap[k]), 1, withheld=(k,))
        assert rec[:, k, 2].sum() == acc.sum_lole - a.sum_lole == s1[k, 2], k
        assert rec[:, k, 3].sum() == acc.sum_eue - a.sum_eue == s1[k, 3], k
        assert 0 < rec[:, k, 2].sum() < rec[:, k, 0].sum()
    ties = 0
    H = load.size
    down0, T, _ = M.chronology(5, [0, 1], mttf, mttr, M.STATIONARY, years * H)
    for c in range(2):
        dn = AM.down_table(down0[c], T[c], years * H)
        cav = sum(np.where(dn[i], 0.0, cap[i]) for i in range(cap.size))
        ties += sum(int(np.sum(dn[k] & (cav + cap[k] == np.tile(load, years)))) for k in range(cap.size))
    assert ties > 0


@pytest.mark.gpu
def test_split_and_repeated_calls(engine):
    cap, mttf, mttr, load = M.fleet100(513)
    K = cap.size
    _load(engine, cap, mttf, mttr, load)
    acc, yr, (s1, s2), rec = _attr(engine, K, 23, 10, 37, 2, M.STATIONARY, 1.02, 1.5)
    acc_b, yr_b, (s1b, s2b), rec_b = _attr(engine, K, 23, 10, 37, 2, M.STATIONARY, 1.02, 1.5)
    assert rec.tobytes() == rec_b.tobytes() and s1.tobytes() == s1b.tobytes() and s2.tobytes() == s2b.tobytes() and _acc_tuple(acc) == _acc_tuple(acc_b)
    # without the host arrays the sums are the same
    _, _, (s1n, s2n), _ = _attr(engine, K, 23, 10, 37, 2, M.STATIONARY, 1.02, 1.5, want_host=False)
    assert s1.tobytes() == s1n.tobytes() and s2.tobytes() == s2n.tobytes()
    lo = _attr(engine, K, 23, 10, 13, 2, M.STATIONARY, 1.02, 1.5)
    hi = _attr(engine, K, 23, 23, 24, 2, M.STATIONARY, 1.02, 1.5)
    assert np.concatenate([lo[3], hi[3]]).tobytes() == rec.tobytes() and np.concatenate([lo[1], hi[1]]).tobytes() == yr.tobytes()
    for q in (0, 2):                                             # the integer fields add exactly
        assert np.array_equal(lo[2][0][:, q] + hi[2][0][:, q], s1[:, q]) and np.array_equal(lo[2][1][:, q] + hi[2][1][:, q], s2[:, q])
    assert s1[:, 0].sum() > 0
    # unit_acc against the fixed-order sums of unit_host
    want1, want2 = np.zeros((K, 4)), np.zeros((K, 4))
    for c in range(rec.shape[0]):
        want1 += rec[c]
        want2 += rec[c] * rec[c]
    np.testing.assert_allclose(s1, want1, rtol=1e-12, atol=0.0)
    np.testing.assert_allclose(s2, want2, rtol=1e-12, atol=0.0)


@pytest.mark.gpu
def test_a_chain_record_does_not_depend_on_its_launch(engine):
    """The chunk rule: a chain counts years_per_chain + (4 * ngen + 2) / 3 records against the 2^22 of a launch, so 100 units and one year
    put 31068 chains into a launch.  The chains on either side of that boundary equal those of a call of their own, and the sums of the
    integer fields are those of the records."""
    cap, mttf, mttr, load = M.fleet100(513)
    K = cap.size
    per = (1 << 22) // (1 + (4 * K + 2) // 3)
    assert per == 31068
    _load(engine, cap, mttf, mttr, load)
    n = per + 5
    acc, yr, (s1, _), rec = _attr(engine, K, 29, 0, n, 1, M.ALL_UP, 1.0, 40.0)
    _, yr_t, _, rec_t = _attr(engine, K, 29, per - 6, 11, 1, M.ALL_UP, 1.0, 40.0)
    assert rec[per - 6:].tobytes() == rec_t.tobytes() and yr[per - 6:].tobytes() == yr_t.tobytes()
    assert rec_t[:, :, 0].sum() > 0
    assert np.array_equal(s1[:, 0], rec[:, :, 0].sum(axis=0)) and np.array_equal(s1[:, 2], rec[:, :, 2].sum(axis=0))
    np.testing.assert_allclose(s1[:, 1], rec[:, :, 1].sum(axis=0), rtol=1e-11)
    assert acc.years == n and acc.sum_lole == yr[:, 0].sum()


@pytest.mark.gpu
def test_small_fleet_against_the_exact_answers(engine):
    """Stationary start, 4096 chains of two years: the four per-unit means within 4.5 of their own standard errors (test_hl1_seq.py's bound
    for its stationary expectations; the errors from unit_acc's sum and sum2) of run_analytical_attribution."""
    cap, mttf, mttr, load = M.small_fleet()
    _load(engine, cap, mttf, mttr, load)
    n, years = 4096, 2
    _, _, (s1, s2), _ = _attr(engine, cap.size, 41, 0, n, years, M.STATIONARY, want_host=False)
    gens = [hl1.Generator(i + 1, float(cap[i]), float(mttf[i]), float(mttr[i])) for i in range(cap.size)]
    an = ha.run_analytical_attribution(gens, hl1.LoadModel(load))
    mean = s1 / n
    se = np.sqrt(np.maximum(s2 / n - mean * mean, 0.0) / (n - 1))
    for q, f in enumerate(ha.FIELDS):
        want = years * getattr(an, f + "_yr")
        print(f, mean[:, q], want, se[:, q])
        assert np.all(se[:, q] > 0) and np.all(np.abs(mean[:, q] - want) < 4.5 * se[:, q]), (f, mean[:, q], want, se[:, q])


@pytest.mark.gpu
def test_error_codes(engine):
    L = engine.L
    h = C.c_void_p()
    assert L.relmc_ctx_create(0, C.byref(h)) == 0
    err = lambda: L.relmc_last_error(h).decode()
    try:
        cap, mttf, mttr, load = M.small_fleet()
        K = cap.size
        acc = _abi.Hl1SeqAcc()
        uacc = (_abi.Hl1AttrAcc * K)()
        yr = np.full((8, 3), -7.0)
        rec = np.full((4, K, 4), -7.0)

        def prefill():
            acc.years, acc.sum_lole = -7, 3.5
            for a in uacc:
                a.sum[0], a.sum2[3] = -7.0, 3.5
            yr[:] = -7.0
            rec[:] = -7.0

        def untouched():
            return (acc.years, acc.sum_lole) == (-7, 3.5) and all((a.sum[0], a.sum2[3]) == (-7.0, 3.5) for a in uacc) and np.all(yr == -7.0) and np.all(rec == -7.0)

        def run(hh=h, n=4, years=2, start=0, scale=1.0, shift=0.0, a=acc, ua=uacc):
            return L.relmc_hl1_attr_seq(hh, 1, 0, n, years, start, scale, shift, None if a is None else C.byref(a), yr.ctypes.data_as(YP), ua,
                                        rec.ctypes.data_as(UP))
        prefill()
        assert run() == -5 and "relmc_hl1_seq_load" in err() and untouched()              # RELMC_ERR_NO_CASE
        assert _load(engine, cap, mttf, mttr, load, h=h) == 0
        for kw in (dict(scale=np.nan), dict(scale=np.inf), dict(shift=-np.inf), dict(shift=np.nan), dict(start=2), dict(start=-1), dict(years=0),
                   dict(n=-1), dict(a=None), dict(ua=None), dict(hh=None)):
            assert run(**kw) == -1, kw
            if "hh" not in kw:
                assert ("scale / shift" in err()) == ("scale" in kw or "shift" in kw), (kw, err())
            assert untouched(), kw
        assert run(n=0) == 0 and acc.years == 0 and acc.sum_lole == 0.0 and all(not any(a.sum) and not any(a.sum2) for a in uacc)
        assert np.all(yr == -7.0) and np.all(rec == -7.0)
        assert run() == 0 and acc.years == 8 and np.all(yr >= 0.0) and np.all(rec >= 0.0)
        # the host arrays are optional
        assert L.relmc_hl1_attr_seq(h, 1, 0, 4, 2, 0, 1.0, 0.0, C.byref(acc), None, uacc, None) == 0 and acc.years == 8
        # the sequential model is left as it was
        a2 = _abi.Hl1SeqAcc()
        assert L.relmc_hl1_seq(h, 1, 0, 4, 2, 0, C.byref(a2), None) == 0 and _acc_tuple(a2) == _acc_tuple(acc)
    finally:
        L.relmc_ctx_destroy(h)


@pytest.mark.gpu
def test_python_layer_on_rts24(engine):
    gens, load = hl1.rts24_generators(), hl1.rts24_load()
    res = ha.run_sequential_attribution(gens, load, 4000, chains=4000, start="stationary", seed=2, engine=engine)
    ref = hl1.run_sequential_mc(gens, load, 4000, chains=4000, start="stationary", seed=2, engine=engine)
    assert res.year_lole.tobytes() == ref.year_lole.tobytes() and res.year_eue.tobytes() == ref.year_eue.tobytes()
    assert (res.lole_hours_yr, res.eue_mwh_yr, res.lolf_occ_yr) == (ref.lole_hours_yr, ref.eue_mwh_yr, ref.lolf_occ_yr)
    K = len(gens)
    assert res.unit_records.shape == (4000, K, 4) and res.importance.shape == (K,)
    assert np.all((res.importance >= 0) & (res.importance <= 1)) and np.all((res.energy_importance >= 0) & (res.energy_importance <= 1))
    assert np.all(res.lole_if_perfect <= res.lole_hours_yr) and np.all(res.eue_if_perfect <= res.eue_mwh_yr) and np.all(res.lole_if_perfect >= 0)
    big = [k for k, g in enumerate(gens) if g.capacity == 400.0]
    assert len(big) == 2 and sorted(np.argsort(-res.importance)[:2].tolist()) == big
    np.testing.assert_allclose(res.importance, res.unit_records[:, :, 0].sum(axis=0) / res.year_lole.sum(), rtol=1e-12)
    np.testing.assert_allclose(res.lole_if_perfect, res.lole_hours_yr - res.unit_records[:, :, 2].sum(axis=0) / 4000, rtol=1e-12)
    assert np.all(res.importance_se > 0) and np.all(res.lole_if_perfect_se > 0) and np.all(res.down_hours_se > 0)
    np.testing.assert_allclose(res.down_hours_se, res.unit_records[:, :, 0].std(axis=0, ddof=1) / np.sqrt(4000), rtol=1e-6)
    an = ha.run_analytical_attribution(gens, load)
    text = ha.attribution_report(res, an)
    print(text)
    first = [r for r in text.splitlines() if r.startswith("1 ")][0]
    assert int(first.split("|")[1]) in big
