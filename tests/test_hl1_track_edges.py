"""The four chronology kernels that came after tests/test_hl1_chrono_edges.py, at the edges where that file runs the earlier ones:
relmc_hl1_var_seq, relmc_hl1_stress_seq, relmc_hl1_ms_seq and relmc_hl1_area_var on years of 1 .. 513 hours (below, at and around a
64-step group, the multi-state kernel's 256-step window and the 512-step window), on 1 .. 128 units (mask words and lane slots full and
one over, a classed or derated unit at each of those edges), with first_chain across 2^32 under picks that see the chain's upper word,
with 0 .. 8 resources (the pair loop and its odd tail), 256 weather years, 8 outage classes, the largest area configuration (8 areas, 128
units, 32 failing ties, 8 resources, 8 storages: 65 024 bytes of dynamic LDS), and in calls that take two launches.  The shapes,
libraries, classes and fleets are tests/tools/hl1_edge_cases.py's; tests/test_hl1_track_edges_host.py ties the models to literal hour
loops on the same shapes, shows from the models' counters that the shapes reach the paths, and that a model with one subtle fault gives
other records.  Tolerances are those of the kernels' own files: counts exact, energies to rel 1e-12 (weather and area-weather) or 1e-9
(stress and multi-state), acc against its own records to rel 1e-12, pins byte for byte."""
import ctypes as C
import functools
import importlib.util
import os

import numpy as np
import pytest

from powersystemsreliabilityassessment_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", "tools", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


E, XM, MM, AVM = (_tool(n) for n in ("hl1_edge_cases", "hl1_stress_model", "hl1_multistate_model", "hl1_area_variable_model"))
VM, SM, SEQ = XM.VM, XM.SM, XM.SEQ

dp, ip = _abi.c_double_p, _abi.c_int32_p
RANDOM, CYCLE = VM.PICK_RANDOM, VM.PICK_CYCLE
ISO, INTER, REF, MAXF = AVM.ISOLATED, AVM.INTERCONNECTED, AVM.REFERENCE, AVM.MAX_FLOW
SHAPES = E.track_shapes()
IDS = [s[0] for s in SHAPES]
MS_SHAPES = E.ms_shapes()
MS_IDS = [s[0] for s in MS_SHAPES]
RS3 = (1.0, 0.5, 1.25)                                                # three resources: the pair and the odd tail
STORAGE_FIELDS = ("sum_lole", "sum_eue", "sum_lolf", "sum_served", "sum_discharged", "sum_charged")
ENERGIES = ("sum_eue", "sum_discharged", "sum_charged")
ACC_FIELDS = [f for f, _ in _abi.Hl1StorageAcc._fields_]
pytestmark = pytest.mark.gpu


# ---- the C ABI, raw ---------------------------------------------------------------------------------------------------------------
def _load(eng, cap, mttf, mttr, load):
    arrs = [np.ascontiguousarray(x, dtype=np.float64) for x in (cap, mttf, mttr, load)]
    eng._check(eng.L.relmc_hl1_seq_load(eng._h, arrs[0].size, *[a.ctypes.data_as(dp) for a in arrs[:3]], arrs[3].size,
                                        arrs[3].ctypes.data_as(dp)), "relmc_hl1_seq_load")
    eng._hl1_seq_loaded = None                     # hl1's cache no longer describes the device


def _var_load(eng, out, wl=None):
    out = np.ascontiguousarray(out, dtype=np.float64)
    nw, nres, H = out.shape
    wl = None if wl is None else np.ascontiguousarray(wl, dtype=np.float64)
    eng._check(eng.L.relmc_hl1_var_load(eng._h, nw, nres, H, out.ctypes.data_as(dp) if out.size else None, None if wl is None else wl.ctypes.data_as(dp)),
               "relmc_hl1_var_load")
    eng._hl1_var_loaded = None                     # hl1_variable's cache no longer describes the device


def _stress_load(eng, mult, cls):
    mult = np.ascontiguousarray(mult, dtype=np.float64)
    cls = np.ascontiguousarray(cls, dtype=np.int32)
    nw, nc, H = mult.shape
    eng._check(eng.L.relmc_hl1_stress_load(eng._h, nw, nc, H, mult.ctypes.data_as(dp), cls.size, cls.ctypes.data_as(ip)), "relmc_hl1_stress_load")
    eng._hl1_stress_loaded = None                  # hl1_stress's cache no longer describes the device


def _track(fn_name, eng, seed, first, n, years, start, storages=(), rs=(), pick=RANDOM):
    """relmc_hl1_var_seq or relmc_hl1_stress_seq -> (acc, yr[n * years, 3], sy[n * years, 3], weather[n * years])."""
    ns = len(storages)
    arr = (_abi.Hl1Storage * max(ns, 1))(*[_abi.Hl1Storage(*s) for s in storages])
    o = _abi.Hl1VarOpts()
    for r, v in enumerate(rs):
        o.resource_scale[r] = v
    o.scale, o.shift, o.pick, o.reserved = 1.0, 0.0, pick, 0
    acc = _abi.Hl1StorageAcc()
    yr, sy, wy = np.zeros((n * years, 3)), np.zeros((n * years, 3)), np.full(n * years, -1, dtype=np.int32)
    eng._check(getattr(eng.L, fn_name)(eng._h, seed, first, n, years, start, C.byref(o), ns, arr if ns else None, C.byref(acc),
                                       yr.ctypes.data_as(C.POINTER(_abi.Hl1SeqYear)), sy.ctypes.data_as(C.POINTER(_abi.Hl1StorageYear)),
                                       wy.ctypes.data_as(ip)), fn_name)
    return acc, yr, sy, wy


_var = functools.partial(_track, "relmc_hl1_var_seq")
_stress = functools.partial(_track, "relmc_hl1_stress_seq")


def _storage(eng, seed, first, n, years, start, storages):
    ns = len(storages)
    arr = (_abi.Hl1Storage * max(ns, 1))(*[_abi.Hl1Storage(*s) for s in storages])
    acc = _abi.Hl1StorageAcc()
    yr, sy = np.zeros((n * years, 3)), np.zeros((n * years, 3))
    eng._check(eng.L.relmc_hl1_seq_storage(eng._h, seed, first, n, years, start, 1.0, 0.0, ns, arr if ns else None, C.byref(acc),
                                           yr.ctypes.data_as(C.POINTER(_abi.Hl1SeqYear)), sy.ctypes.data_as(C.POINTER(_abi.Hl1StorageYear))),
               "relmc_hl1_seq_storage")
    return acc, yr, sy


def _seq(eng, seed, first, n, years, start):
    acc = _abi.Hl1SeqAcc()
    yr = np.zeros((n * years, 3))
    eng._check(eng.L.relmc_hl1_seq(eng._h, seed, first, n, years, start, C.byref(acc), yr.ctypes.data_as(C.POINTER(_abi.Hl1SeqYear))),
               "relmc_hl1_seq")
    return acc, yr


def _ms_load(eng, units, load):
    ld = np.ascontiguousarray(load, dtype=np.float64)
    arr = (_abi.Hl1MsUnit * len(units))(*[_abi.Hl1MsUnit(u[0], u[1], (C.c_double * 3)(*u[2]), (C.c_double * 3)(*u[3])) for u in units])
    eng._check(eng.L.relmc_hl1_ms_load(eng._h, len(units), arr, ld.size, ld.ctypes.data_as(dp)), "relmc_hl1_ms_load")
    eng._hl1_ms_loaded = None                      # hl1_multistate's cache no longer describes the device


def _ms(eng, seed, first, n, years, start):
    acc = _abi.Hl1MsAcc()
    yr, sy = np.zeros((n * years, 3)), np.zeros((n * years, 2))
    eng._check(eng.L.relmc_hl1_ms_seq(eng._h, seed, first, n, years, start, C.byref(acc), yr.ctypes.data_as(C.POINTER(_abi.Hl1SeqYear)),
                                      sy.ctypes.data_as(C.POINTER(_abi.Hl1MsYear))), "relmc_hl1_ms_seq")
    return acc, yr, sy


def _acc_tuple(a):
    return tuple(getattr(a, f) for f, _ in type(a)._fields_)


def _same(a, b):
    """Two calls of the track entry points gave the same bytes: both record rows, acc and the weather years."""
    return a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes() and _acc_tuple(a[0]) == _acc_tuple(b[0]) and \
        (len(a) < 4 or len(b) < 4 or np.array_equal(a[3], b[3]))


def _assert_track_equals_model(got, rec, W, rtol):
    """Counts exact, the three energies to rtol, weather_host the model's weather years, acc the sum of its own records (counts exactly,
    energies to rel 1e-12)."""
    acc, yr, sy, wy = got
    np.testing.assert_array_equal(wy, W)
    np.testing.assert_array_equal(yr[:, 0], rec[:, 0])
    np.testing.assert_array_equal(yr[:, 2], rec[:, 2])
    np.testing.assert_array_equal(sy[:, 0], rec[:, 3])
    print("max rel diff of the energies", [float(np.max(np.abs(a - b) / np.where(b == 0.0, 1.0, b), initial=0.0)) for a, b in
                                           ((yr[:, 1], rec[:, 1]), (sy[:, 1], rec[:, 4]), (sy[:, 2], rec[:, 5]))])
    np.testing.assert_allclose(yr[:, 1], rec[:, 1], rtol=rtol, atol=0.0)
    np.testing.assert_allclose(sy[:, 1], rec[:, 4], rtol=rtol, atol=0.0)
    np.testing.assert_allclose(sy[:, 2], rec[:, 5], rtol=rtol, atol=0.0)
    assert acc.years == yr.shape[0]
    _assert_acc_is_the_sum_of_its_records(acc, np.concatenate([yr, sy], axis=1))


def _assert_acc_is_the_sum_of_its_records(acc, rec):
    for q, f in enumerate(STORAGE_FIELDS):
        want = (rec[:, q].sum(), (rec[:, q] ** 2).sum())
        if f in ENERGIES:
            want = tuple(pytest.approx(w, rel=1e-12) for w in want)
        assert (getattr(acc, f), getattr(acc, f + "2")) == want, f


def _assert_acc_is_the_sum_of_two(acc, acc1, acc2):
    assert acc.years == acc1.years + acc2.years
    for f in STORAGE_FIELDS:
        for g in (f, f + "2"):
            if f in ENERGIES:
                assert getattr(acc, g) == pytest.approx(getattr(acc1, g) + getattr(acc2, g), rel=1e-12), g
            else:
                assert getattr(acc, g) == getattr(acc1, g) + getattr(acc2, g), g


# ---- a. the pins, device against device --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_weather_track_with_nothing_added_is_the_storage_kernel(engine, shape):
    """A library of three resources all scaled 0 and no load curves, with edge_storages: both record rows and acc are
    relmc_hl1_seq_storage's byte for byte, whatever weather years are drawn."""
    label, (cap, mttf, mttr, load), seed, first, n, years, start, pick = shape
    st = E.edge_storages(cap)
    _load(engine, cap, mttf, mttr, load)
    _var_load(engine, E.edge_weather(load, 3, 3, False)[0])
    got = _var(engine, seed, first, n, years, start, st, (0.0, 0.0, 0.0), pick)
    want = _storage(engine, seed, first, n, years, start, st)
    assert _same(got, want) and want[1][:, 0].sum() > 0 and want[2][:, 1].sum() > 0          # loss hours, and the storages deliver
    assert np.array_equal(got[3], VM.weather_years(seed, range(first, first + n), years, 3, pick).reshape(-1))


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_stress_track_with_every_unit_in_class_minus_one_is_the_weather_kernel(engine, shape):
    """The edge library with curves and storages, edge_stress loaded but every unit in class -1: relmc_hl1_var_seq byte for byte."""
    label, (cap, mttf, mttr, load), seed, first, n, years, start, pick = shape
    st = E.edge_storages(cap)
    _load(engine, cap, mttf, mttr, load)
    _var_load(engine, *E.edge_weather(load, 3, 3, True))
    _stress_load(engine, E.edge_stress(3, 3, len(load)), [-1] * len(cap))
    args = (engine, seed, first, n, years, start, st, RS3, pick)
    got, want = _stress(*args), _var(*args)
    assert _same(got, want) and want[1][:, 0].sum() > 0 and want[2][:, 0].sum() > 0


@pytest.mark.parametrize("shape", MS_SHAPES, ids=MS_IDS)
def test_multistate_on_the_two_state_image_is_the_sequential_kernel(engine, shape):
    """Every unit with first_p (1, 1, 1): relmc_hl1_seq's records and sums byte for byte, on 8 units at MS_NHOURS_EDGES (the kernel's
    256-step window, and the 512-step window of the kernel it is pinned to) and on NGEN_EDGES."""
    label, fleet, seed, first, n, years, start = shape
    _, two, load = E.ms_fleet(*fleet)
    cap, mttf, mttr, _ = E.seq_fleet(*fleet)
    _load(engine, cap, mttf, mttr, load)
    _ms_load(engine, two, load)
    acc0, want = _seq(engine, seed, first, n, years, start)
    acc, yr, sy = _ms(engine, seed, first, n, years, start)
    assert yr.tobytes() == want.tobytes() and want[:, 0].sum() > 0
    assert _acc_tuple(acc)[:7] == _acc_tuple(acc0) and not sy[:, 0].any() and (fleet[0] == 1 and label.endswith("-0") or sy[:, 1].sum() > 0)


# ---- b. the weather track against its model -------------------------------------------------------------------------------------------------
def _weather_model(shape, n_weather=3, n_res=3, pick=None, n=None):
    label, (cap, mttf, mttr, load), seed, first, n0, years, start, pick0 = shape
    n, pick = n or n0, pick0 if pick is None else pick
    out, wl = E.edge_weather(load, n_weather, n_res, True)
    rs = (RS3 + (0.0, 1.0, 0.75, 1.0, 2.0))[:n_res]
    st = E.edge_storages(cap)
    cnt = SM.new_counters()
    rec, W = VM.variable_model(seed, range(first, first + n), cap, mttf, mttr, load, years, start, out, wl, rs, pick, st, counters=cnt)
    return out, wl, rs, st, rec, W, cnt, n, pick


def _run_weather(engine, shape, **kw):
    label, (cap, mttf, mttr, load), seed, first, _, years, start, _ = shape
    out, wl, rs, st, rec, W, cnt, n, pick = _weather_model(shape, **kw)
    _load(engine, cap, mttf, mttr, load)
    _var_load(engine, out, wl)
    got = _var(engine, seed, first, n, years, start, st, rs, pick)
    _assert_track_equals_model(got, rec, W, 1e-12)
    return got, rec, W, cnt


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_weather_track_equals_the_host_model(engine, shape):
    """Three weather years with curves, three resources (the odd tail of the resource loop), edge_storages; RANDOM on the all-UP shapes,
    CYCLE on the stationary ones.  The shape reaches its paths (track_coverage)."""
    got, rec, W, cnt = _run_weather(engine, shape)
    E.track_coverage(shape[0], cnt, W, len(shape[1][3]), shape[5])


@pytest.mark.parametrize("n_res", [0, 1, 2, 3, 4, 7, 8])
def test_weather_track_resource_counts(engine, n_res):
    """H = 65 with 0 .. 8 resources: none (a library that has load curves only), the two read ahead, pairs, and the odd tails 3 and 7.
    With four resources or more one of them is scaled 0."""
    shape = SHAPES[IDS.index("h65-0")]
    got, rec, W, cnt = _run_weather(engine, shape, n_res=n_res)
    assert cnt["lost"] > 0 and cnt["served"] > 0 and sum(cnt["charge"]) > 0
    if n_res:                                                         # the last resource counts: without it the model has other records
        label, (cap, mttf, mttr, load), seed, first, n, years, start, pick = shape
        out, wl, rs, st = _weather_model(shape, n_res=n_res)[:4]
        if rs[-1] == 0.0:
            return
        less, _ = VM.variable_model(seed, range(first, first + n), cap, mttf, mttr, load, years, start, out, wl, rs[:-1] + (0.0,), pick, st)
        assert not np.array_equal(less[:, [0, 3]], rec[:, [0, 3]])


@pytest.mark.parametrize("pick", [RANDOM, CYCLE])
def test_weather_track_with_256_weather_years(engine, pick):
    """n_weather = 256 at H = 24 with curves and two resources: 48 chains of 67 years, in which every weather year occurs."""
    shape = SHAPES[IDS.index("h24-0" if pick == RANDOM else "h24-1")]
    got, rec, W, cnt = _run_weather(engine, shape, n_weather=256, n_res=2, pick=pick, n=48)
    assert np.unique(got[3]).size == 256 and cnt["lost"] > 0 and cnt["served"] > 0


# ---- c. the stress track against its model -------------------------------------------------------------------------------------------------
def _run_stress(engine, shape, n_weather=3, n_classes=3, pick=None):
    label, (cap, mttf, mttr, load), seed, first, n, years, start, pick0 = shape
    pick = pick0 if pick is None else pick
    out, wl = E.edge_weather(load, n_weather, 3, True)
    st = E.edge_storages(cap)
    mult, cls = E.edge_stress(n_weather, n_classes, len(load)), E.edge_classes(len(cap), n_classes)
    cnt, steps = {}, SM.new_counters()
    rec, W = XM.stress_model(seed, range(first, first + n), cap, mttf, mttr, load, years, start, out, mult, cls, wl, RS3, pick, st, counters=cnt,
                             step_counters=steps)
    _load(engine, cap, mttf, mttr, load)
    _var_load(engine, out, wl)
    _stress_load(engine, mult, cls)
    got = _stress(engine, seed, first, n, years, start, st, RS3, pick)
    _assert_track_equals_model(got, rec, W, 1e-9)
    return got, rec, W, cnt, steps, cls


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_stress_track_equals_the_host_model(engine, shape):
    """edge_stress with three classes (zero stretches, a zero year, spikes with landings on the flat hours between them, a class that
    never fails) and edge_classes (a classed unit at 0, 31, 32, 63, 64 and 127, class -1 beside each).  The shape reaches its paths
    (track_coverage, stress_coverage), and relmc_hl1_var_seq gives other records on the same data."""
    label, (cap, mttf, mttr, load), seed, first, n, years, start, pick = shape
    got, rec, W, cnt, steps, cls = _run_stress(engine, shape)
    E.track_coverage(label, steps, W, len(load), years)
    E.stress_coverage(label, cnt, len(load), len(cap))
    ref = _var(engine, seed, first, n, years, start, E.edge_storages(cap), RS3, pick)
    assert np.array_equal(ref[3], got[3]) and ref[1].tobytes() != got[1].tobytes()


def test_stress_track_with_eight_classes(engine):
    """n_classes = 8 on 128 units (both lane slots), across first_chain = 2^32: every class is used."""
    shape = SHAPES[IDS.index("g128-1")]
    got, rec, W, cnt, steps, cls = _run_stress(engine, shape, n_classes=8)
    assert set(cls.tolist()) == set(range(-1, 8)) and cnt["flat"] > 0 and cnt["immediate"] > 0 and cnt["carried"] > 0


# ---- d. the multi-state kernel against its model ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", MS_SHAPES, ids=MS_IDS)
def test_multistate_equals_the_host_model(engine, shape):
    """ms_fleet (derated units at 0, 31, 32, 63, 64 and 127, branch probabilities of 0, of 1 and strictly inside in every state) on 8
    units at MS_NHOURS_EDGES under both start rules, and on NGEN_EDGES at H = 100 from chain 0 and across 2^32: every count exact, EUE to
    1e-9 (tests/test_hl1_multistate.py's rule), acc against its own records.  The shape reaches its paths (ms_coverage)."""
    label, fleet, seed, first, n, years, start = shape
    units, _, load = E.ms_fleet(*fleet)
    chains = range(first, first + n)
    E.ms_coverage(label, fleet[1], MM.path_counts(seed, chains, units, load, years, start))
    _ms_load(engine, units, load)
    acc, yr, sy = _ms(engine, seed, first, n, years, start)
    rec = MM.interval_model(seed, chains, units, load, years, start)
    np.testing.assert_array_equal(yr[:, 0], rec[:, 0])
    np.testing.assert_array_equal(yr[:, 2], rec[:, 2])
    np.testing.assert_array_equal(sy[:, 0], rec[:, 3])
    np.testing.assert_array_equal(sy[:, 1], rec[:, 4])
    np.testing.assert_allclose(yr[:, 1], rec[:, 1], rtol=1e-9, atol=0.0)
    assert acc.years == n * years and rec[:, 0].sum() > 0 and rec[:, 3].sum() > 0 and rec[:, 4].sum() > 0
    both = np.concatenate([yr, sy], axis=1)
    for q, f in ((0, "sum_lole"), (1, "sum_eue"), (2, "sum_lolf"), (3, "sum_derated"), (4, "sum_down")):
        assert getattr(acc, f) == pytest.approx(both[:, q].sum(), rel=1e-12), f
        assert getattr(acc, f + "2") == pytest.approx((both[:, q] ** 2).sum(), rel=1e-12), f


# ---- e. chains across 2^32 under picks that see the upper word ---------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [s for s in SHAPES if s[0].startswith("g") and s[0].endswith("-1")], ids=lambda s: s[0])
def test_weather_picks_across_2_32(engine, shape):
    """The g*-1 shapes (first_chain = 2^32 - 4) under RANDOM over 3 and CYCLE over 5 weather years (UPPER_WORD_PICKS): chain 2^32 + j has
    other weather years than chain j there (tests/test_hl1_track_edges_host.py shows it, and that the model's records change with them),
    so a device pick without the upper word fails these comparisons, on the weather and on the stress track."""
    for pick, nw in E.UPPER_WORD_PICKS:
        _run_weather(engine, shape, n_weather=nw, pick=pick)
        _run_stress(engine, shape, n_weather=nw, pick=pick)


# ---- f. the area-weather kernel -----------------------------------------------------------------------------------------------------------------
def _area_load(eng, c, outages=True):
    u = np.ascontiguousarray(c["units"], dtype=np.int32)
    ties = c["ties"]
    arrs = [np.ascontiguousarray(x, dtype=np.float64) for x in (c["cap"], c["mttf"], c["mttr"], c["loads"], [t[2] for t in ties], c["tie_mttf"],
                                                                c["tie_mttr"])]
    tf, tt = (np.ascontiguousarray([t[i] for t in ties], dtype=np.int32) for i in (0, 1))
    eng._check(eng.L.relmc_hl1_area_load(eng._h, u.size, u.ctypes.data_as(ip), *[a.ctypes.data_as(dp) for a in arrs[:3]], arrs[3].shape[-1],
                                         arrs[3].ctypes.data_as(dp), tf.size, tf.ctypes.data_as(ip), tt.ctypes.data_as(ip),
                                         arrs[4].ctypes.data_as(dp)), "relmc_hl1_area_load")
    if outages:
        eng._check(eng.L.relmc_hl1_area_tie_outages(eng._h, arrs[5].size, arrs[5].ctypes.data_as(dp), arrs[6].ctypes.data_as(dp)),
                   "relmc_hl1_area_tie_outages")
    eng._hl1_area_loaded = None                    # hl1_areas' cache no longer describes the device


def _lib_load(eng, n_areas, out, rarea, wl=None):
    out = np.ascontiguousarray(out, dtype=np.float64)
    nw, nres, H = out.shape
    ra = np.ascontiguousarray(rarea, dtype=np.int32)
    wl = None if wl is None else np.ascontiguousarray(wl, dtype=np.float64)
    eng._check(eng.L.relmc_hl1_area_var_load(eng._h, n_areas, nw, nres, ra.ctypes.data_as(ip) if ra.size else None, H,
                                             out.ctypes.data_as(dp) if out.size else None, None if wl is None else wl.ctypes.data_as(dp)),
               "relmc_hl1_area_var_load")
    eng._hl1_area_var_loaded = None                # hl1_area_variable's cache no longer describes the device


def _area_var(eng, rows, seed, first, n, years, start, policy, flow, rs=(), storages=(), pick=RANDOM):
    """-> (acc[rows], yr[n * years, rows, 3], sy[n * years, rows, 3], weather[n * years], rc); storages: (area0, six fields).  The return
    code is returned, not checked: the largest configuration's is what its test is about."""
    o = _abi.Hl1AreaVarOpts()
    for a in range(_abi.AREA_MAX):
        o.load_scale[a], o.load_shift[a] = 1.0, 0.0
    for r, v in enumerate(rs):
        o.resource_scale[r] = v
    o.policy, o.flow, o.pick, o.reserved = policy, flow, pick, 0
    ns = len(storages)
    arr = (_abi.Hl1AreaStorage * max(ns, 1))()
    for i, (a, s) in enumerate(storages):
        arr[i].s = _abi.Hl1Storage(*s)
        arr[i].area, arr[i].reserved = a, 0
    acc = (_abi.Hl1StorageAcc * rows)()
    yr, sy, wy = np.full((n * years, rows, 3), -7.0), np.full((n * years, rows, 3), -7.0), np.full(n * years, -1, dtype=np.int32)
    rc = eng.L.relmc_hl1_area_var(eng._h, seed, first, n, years, start, C.byref(o), ns, arr if ns else None, acc,
                                  yr.ctypes.data_as(C.POINTER(_abi.Hl1SeqYear)), sy.ctypes.data_as(C.POINTER(_abi.Hl1StorageYear)), wy.ctypes.data_as(ip))
    return acc, yr, sy, wy, rc


def _area(eng, rows, seed, first, n, years, start, policy, flow):
    acc = (_abi.Hl1SeqAcc * rows)()
    yr = np.zeros((n * years, rows, 3))
    eng._check(eng.L.relmc_hl1_area(eng._h, seed, first, n, years, start, policy, flow, acc, yr.ctypes.data_as(C.POINTER(_abi.Hl1SeqYear))),
               "relmc_hl1_area")
    return acc, yr


def _area_model(c, seed, chains, years, start, policy, flow, storages, pick=RANDOM, counters=None):
    return AVM.area_variable_model(seed, chains, c["units"], c["cap"], c["mttf"], c["mttr"], c["loads"], c["ties"], years, start, policy, flow,
                                   c["out"], c["resource_area"], c["wl"], c["resource_scale"], pick=pick, storages=storages,
                                   tie_mttf=c["tie_mttf"], tie_mttr=c["tie_mttr"], counters=counters)


def _assert_area_equals_model(got, model, W):
    """tests/test_hl1_area_variable.py's rule: counts exact, energies to rel 1e-12, acc against its own records."""
    acc, yr, sy, wy, rc = got
    assert rc == 0
    np.testing.assert_array_equal(wy, W)
    np.testing.assert_array_equal(yr[..., 0], model[..., 0])
    np.testing.assert_array_equal(yr[..., 2], model[..., 2])
    np.testing.assert_array_equal(sy[..., 0], model[..., 3])
    np.testing.assert_allclose(yr[..., 1], model[..., 1], rtol=1e-12, atol=0.0)
    np.testing.assert_allclose(sy[..., 1], model[..., 4], rtol=1e-12, atol=0.0)
    np.testing.assert_allclose(sy[..., 2], model[..., 5], rtol=1e-12, atol=0.0)
    for r in range(yr.shape[1]):
        assert acc[r].years == yr.shape[0]
        _assert_acc_is_the_sum_of_its_records(acc[r], np.concatenate([yr[:, r], sy[:, r]], axis=1))


@pytest.mark.parametrize("nhours", [48, 513])
def test_area_weather_largest_configuration(engine, nhours):
    """area_var_max_case: 8 areas, 128 units, 32 failing ties, 8 resources, 8 storages, load curves per weather year.  INTERCONNECTED
    with storages is the largest dynamic LDS the entry point asks for (107 rows of 512 bytes and five mask rows: 65 024 of the 65 536
    bytes a launch gets without raising the limit); the call returns RELMC_OK and equals the model.  So do the three other LDS layouts
    (ISOLATED / INTERCONNECTED, with / without storages) and, with storages, both flows.  With nothing added (resources scaled 0, a library without
    curves, no storage) the loss records are relmc_hl1_area's byte for byte."""
    c = E.area_var_max_case(nhours)
    years, n, first, seed, start = E.seq_years(nhours), 2, 2, 17, AVM.STATIONARY
    _area_load(engine, c)
    _lib_load(engine, 8, c["out"], c["resource_area"], c["wl"])
    seen = np.zeros(6)
    with_st = c["storages"]
    for policy, flow, st in ((INTER, MAXF, with_st), (INTER, REF, with_st), (ISO, REF, with_st), (INTER, MAXF, []), (ISO, REF, [])):
        got = _area_var(engine, 9, seed, first, n, years, start, policy, flow, c["resource_scale"], st)
        assert got[4] == 0, engine.L.relmc_last_error(engine._h).decode()           # RELMC_OK: the launch is not refused
        model, W = _area_model(c, seed, range(first, first + n), years, start, policy, flow, st)
        _assert_area_equals_model(got, model, W)
        seen += model[:, 8].sum(0)
        if not st:
            assert not got[2].any()
    assert seen[0] > 0 and seen[3] > 0 and seen[4] > 0 and seen[5] > 0         # loss, served, discharging and charging steps occur
    _lib_load(engine, 8, c["out"], c["resource_area"])
    for policy, flow in ((INTER, MAXF), (INTER, REF), (ISO, REF)):
        acc0, want = _area(engine, 9, seed, first, n, years, start, policy, flow)
        acc, yr, sy, wy, rc = _area_var(engine, 9, seed, first, n, years, start, policy, flow, [0.0] * 8)
        assert rc == 0 and yr.tobytes() == want.tobytes() and not sy.any() and want[:, 8, 0].sum() > 0
        assert [_acc_tuple(a)[:7] for a in acc] == [_acc_tuple(a) for a in acc0]


@pytest.mark.parametrize("nhours", [1, 63, 64, 65, 511, 512, 513])
def test_area_weather_at_the_year_edges(engine, nhours):
    """area_tie_edges(65, nhours) (4 areas, two unit slots, 32 failing ties) with 3 resources (the odd tail) and 2 storages, from chain 0
    under REFERENCE and RANDOM and across 2^32 under MAX_FLOW and CYCLE, against the model."""
    c = E.area_var_tie_case(65, nhours)
    years = E.seq_years(nhours)
    _area_load(engine, c)
    _lib_load(engine, 4, c["out"], c["resource_area"], c["wl"])
    for first, flow, pick, start in ((0, REF, RANDOM, AVM.ALL_UP), ((1 << 32) - 2, MAXF, CYCLE, AVM.STATIONARY)):
        got = _area_var(engine, 5, 17, first, 4, years, start, INTER, flow, c["resource_scale"], c["storages"], pick)
        model, W = _area_model(c, 17, range(first, first + 4), years, start, INTER, flow, c["storages"], pick)
        _assert_area_equals_model(got, model, W)
        assert model[:, 4, 0].sum() > 0 and model[:, 4, 4].sum() > 0 and np.unique(W).size == 3


# ---- g. two launches ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("track", ["weather", "stress"])
def test_track_two_launches(engine, track):
    """2100 chains x 1000 years of 24 hours with 3 weather years and 2 storages: a launch holds 2^22 / (1000 * 2) = 2097 chains, so the
    second has three, another record stride and another first chain.  Both rows and weather_host against two calls split at the cut
    (bitwise), the six chains around the cut against the model, acc against the two calls' sums and against its own records."""
    cap, mttf, mttr, load = E.seq_fleet(6, 24)
    N, Y = 2100, 1000
    st = E.edge_storages(cap)[:2]
    out, wl = E.edge_weather(load, 3, 3, True)
    per = E.RECORD_BUDGET // (Y * 2)
    assert per == 2097 and per < N < 2 * per
    _load(engine, cap, mttf, mttr, load)
    _var_load(engine, out, wl)
    run = _var
    w0, w1 = per - 3, per + 3
    if track == "stress":
        mult, cls = E.edge_stress(3, 3, 24), E.edge_classes(6)
        _stress_load(engine, mult, cls)
        run = _stress
        rec, W = XM.stress_model(8, range(w0, w1), cap, mttf, mttr, load, Y, SEQ.STATIONARY, out, mult, cls, wl, RS3, RANDOM, st)
    else:
        rec, W = VM.variable_model(8, range(w0, w1), cap, mttf, mttr, load, Y, SEQ.STATIONARY, out, wl, RS3, RANDOM, st)
    assert rec[:, 0].sum() > 0 and rec[:, 3].sum() > 0 and rec[:, 5].sum() > 0
    acc, yr, sy, wy = run(engine, 8, 0, N, Y, SEQ.STATIONARY, st, RS3, RANDOM)
    got = np.concatenate([yr[w0 * Y:w1 * Y], sy[w0 * Y:w1 * Y]], axis=1)
    np.testing.assert_array_equal(wy[w0 * Y:w1 * Y], W)
    np.testing.assert_array_equal(got[:, [0, 2, 3]], rec[:, [0, 2, 3]])
    np.testing.assert_allclose(got[:, [1, 4, 5]], rec[:, [1, 4, 5]], rtol=1e-12 if track == "weather" else 1e-9, atol=0.0)
    acc1, yr1, sy1, wy1 = run(engine, 8, 0, per, Y, SEQ.STATIONARY, st, RS3, RANDOM)
    acc2, yr2, sy2, wy2 = run(engine, 8, per, N - per, Y, SEQ.STATIONARY, st, RS3, RANDOM)
    assert np.array_equal(yr[:per * Y], yr1) and np.array_equal(yr[per * Y:], yr2)
    assert np.array_equal(sy[:per * Y], sy1) and np.array_equal(sy[per * Y:], sy2)
    assert np.array_equal(wy[:per * Y], wy1) and np.array_equal(wy[per * Y:], wy2) and np.unique(wy2).size == 3
    assert sy2[:, 0].sum() > 0 and sy2[:, 2].sum() > 0 and yr2.tobytes() != sy2.tobytes()
    assert acc.years == N * Y
    _assert_acc_is_the_sum_of_two(acc, acc1, acc2)
    _assert_acc_is_the_sum_of_its_records(acc, np.concatenate([yr, sy], axis=1))


def test_area_weather_two_launches(engine):
    """hl1_area_variable_model's two-area shape (6 units, a 24-hour year, one failing tie, 2 resources, 2 storages) with 702 chains x 1000
    years: three rows of two records each, so a launch holds 2^22 / (6 * 1000) = 699 chains and the second has three.  Both records and
    weather_host against two calls split at the cut (bitwise), the two chains around the cut against the model, acc against the two
    calls' sums and against its own records."""
    s = AVM.shape("a2")
    out, wl = AVM.library(s["loads"], 3, s["resource_area"], 11, True)
    c = dict(s, out=out, wl=wl)
    N, Y = 702, 1000
    per = E.RECORD_BUDGET // (6 * Y)
    assert per == 699 and per < N < 2 * per
    _area_load(engine, c)
    _lib_load(engine, 2, out, s["resource_area"], wl)
    args = (Y, AVM.STATIONARY, INTER, MAXF, s["resource_scale"], s["storages"], CYCLE)
    acc, yr, sy, wy, rc = _area_var(engine, 3, 8, 0, N, *args)
    assert rc == 0
    w0, w1 = per - 1, per + 1
    model, W = _area_model(c, 8, range(w0, w1), Y, AVM.STATIONARY, INTER, MAXF, s["storages"], CYCLE)
    assert model[:, 2, 0].sum() > 0 and model[:, 2, 3].sum() > 0 and model[:, 2, 5].sum() > 0
    np.testing.assert_array_equal(wy[w0 * Y:w1 * Y], W)
    np.testing.assert_array_equal(yr[w0 * Y:w1 * Y][..., [0, 2]], model[..., [0, 2]])
    np.testing.assert_array_equal(sy[w0 * Y:w1 * Y][..., 0], model[..., 3])
    np.testing.assert_allclose(yr[w0 * Y:w1 * Y][..., 1], model[..., 1], rtol=1e-12, atol=0.0)
    np.testing.assert_allclose(sy[w0 * Y:w1 * Y][..., 1:], model[..., 4:], rtol=1e-12, atol=0.0)
    acc1, yr1, sy1, wy1, rc1 = _area_var(engine, 3, 8, 0, per, *args)
    acc2, yr2, sy2, wy2, rc2 = _area_var(engine, 3, 8, per, N - per, *args)
    assert rc1 == 0 and rc2 == 0
    assert np.array_equal(yr[:per * Y], yr1) and np.array_equal(yr[per * Y:], yr2)
    assert np.array_equal(sy[:per * Y], sy1) and np.array_equal(sy[per * Y:], sy2)
    assert np.array_equal(wy[:per * Y], wy1) and np.array_equal(wy[per * Y:], wy2) and np.unique(wy2).size == 3
    assert sy2[..., 0].sum() > 0 and sy2[..., 2].sum() > 0
    for r in range(3):
        assert acc[r].years == N * Y
        _assert_acc_is_the_sum_of_two(acc[r], acc1[r], acc2[r])
        _assert_acc_is_the_sum_of_its_records(acc[r], np.concatenate([yr[:, r], sy[:, r]], axis=1))
