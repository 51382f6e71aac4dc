"""The host side of tests/test_hl1_track_edges.py (no GPU): the weather, stress and multi-state models against their literal hour loops on
shapes of tests/tools/hl1_edge_cases.py (years of 1, 64, 65 and 513 hours; 1, 65 and 128 units), the paths every shape reaches, read off
the models' own counters (a shape that stops exercising a path fails here, before any GPU run), and the proof that each comparison of
the device test can fail: a model that drops the chain's upper word, skips the odd-tail resource or reads class k for unit k + 64 gives
other records on the cases."""
import functools
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", "tools", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


E, XM, MM, AVM = (_tool(n) for n in ("hl1_edge_cases", "hl1_stress_model", "hl1_multistate_model", "hl1_area_variable_model"))
VM, SM, SEQ = XM.VM, XM.SM, XM.SEQ
SHAPES = E.track_shapes()
IDS = [s[0] for s in SHAPES]
MS_SHAPES = E.ms_shapes()
MS_IDS = [s[0] for s in MS_SHAPES]
LITERAL = ("h1-0", "h1-1", "h64-0", "h65-1", "h513-0", "g1-1", "g65-0", "g128-1")      # H = 1, 64, 65, 513 and 1, 65, 128 units
RS3 = (1.0, 0.5, 1.25)                                                                # three resources: the pair and the odd tail


def _shape(label):
    return SHAPES[IDS.index(label)]


def _middle(first):
    """The four middle chains of a shape's eight, which the literal loops run (on the g*-1 shapes two on either side of 2^32)."""
    return range(first + 2, first + 6)


@functools.lru_cache(maxsize=None)
def _weather_case(label, pick=None, nw=3):
    """The weather case of a shape as the device test runs it, with the model's records, weather years and step counters."""
    _, (cap, mttf, mttr, load), seed, first, n, years, start, pick0 = _shape(label)
    pick = pick0 if pick is None else pick
    out, wl = E.edge_weather(load, nw, 3, True)
    st = E.edge_storages(cap)
    cnt = SM.new_counters()
    rec, W = VM.variable_model(seed, range(first, first + n), cap, mttf, mttr, load, years, start, out, wl, RS3, pick, st, counters=cnt)
    rec.setflags(write=False)
    return out, wl, st, rec, W, cnt


@functools.lru_cache(maxsize=None)
def _stress_case(label, pick=None, nw=3):
    _, (cap, mttf, mttr, load), seed, first, n, years, start, pick0 = _shape(label)
    pick = pick0 if pick is None else pick
    out, wl = E.edge_weather(load, nw, 3, True)
    st = E.edge_storages(cap)
    mult, cls = E.edge_stress(nw, 3, len(load)), E.edge_classes(len(cap))
    cnt, steps = {}, SM.new_counters()
    rec, W = XM.stress_model(seed, range(first, first + n), cap, mttf, mttr, load, years, start, out, mult, cls, wl, RS3, pick, st, counters=cnt,
                             step_counters=steps)
    rec.setflags(write=False)
    return out, wl, st, mult, cls, rec, W, cnt, steps


# ---- the cases themselves -----------------------------------------------------------------------------------------------------------------
def test_edge_libraries_are_what_they_say():
    for H in E.NHOURS_EDGES + (100,):
        load = E.seq_fleet(8, H)[3]
        for nw, nres in ((3, 3), (1, 1), (256, 8), (3, 0)):
            out, wl = E.edge_weather(load, nw, nres, True)
            assert out.shape == (nw, nres, H) and wl.shape == (nw, H) and np.array_equal(out * 64.0, np.floor(out * 64.0)) and out.min(initial=0.0) >= 0.0
            assert out.sum(axis=1).max(initial=0.0) <= 0.12 * abs(load.mean())
            if nres:
                assert not out[min(1, nw - 1), nres - 1].any() and all(out[w].any() for w in range(nw) if w != min(1, nw - 1) or nres > 1)
            assert nw == 1 or len({wl[w].tobytes() for w in range(nw)}) == nw
            assert E.edge_weather(load, nw, nres, False)[1] is None
        for nc in (3, 8):
            m = E.edge_stress(3, nc, H)
            assert m.shape == (3, nc, H) and m.min() >= 0.0 and np.array_equal(m * 2.0 ** 24, np.floor(m * 2.0 ** 24))
            assert not m[1, 0].any() and XM.cumulative(m[1, 0])[H] == 0.0          # the zero row
            assert m[2, 1].max() == E.SPIKE and np.all(m[:, 2] == 2.0 ** -24)
            if H == 1:
                assert m[0, 0, 0] > 0.0 and m[1, 0, 0] == 0.0
            else:
                sp = E.spike_hours(H)
                assert len(sp) >= 3 and np.all(m[2, 1, sp] == E.SPIKE) and m[2, 1].sum() == len(sp) * E.SPIKE
                assert all(not m[0, 0, s].any() for s in (slice(0, 1), slice(H // 2, H // 2 + 1), slice(H - 1, H)))
                assert all(np.any(m[:, c] == 0.0) and np.any(m[:, c] > 0.0) for c in range(3, nc))
    assert E.SPIKE + 127.0 == E.SPIKE and E.SPIKE + 129.0 > E.SPIKE
    for ngen in E.NGEN_EDGES + (8,):
        for nc in (3, 8):
            cls = E.edge_classes(ngen, nc)
            edge = [k for k in E.EDGE_UNITS if k < ngen]
            assert cls.shape == (ngen,) and cls.min() >= -1 and cls.max() < nc and all(cls[k] >= 0 for k in edge)
            assert all(cls[nb] == -1 for k in edge for nb in (k - 1, k + 1) if 0 <= nb < ngen and nb not in edge)
            if ngen >= nc + 3:
                assert set(cls.tolist()) == set(range(-1, nc)), (ngen, nc)
    assert E.edge_classes(1)[0] == 1 and E.edge_classes(8)[2] == 1                   # the one-unit fleet and the fast unit are in the spike class
    for ngen in E.NGEN_EDGES + (8,):
        units, two, load = E.ms_fleet(ngen, 100)
        cap, mttf, mttr, ld = E.seq_fleet(ngen, 100)
        assert [u[0] for u in units] == cap.tolist() == [u[0] for u in two] and np.array_equal(load, ld)
        assert all(u[3] == (1.0, 1.0, 1.0) and u[2] == (mttf[k], 1.0, mttr[k]) for k, u in enumerate(two))
        der = [k for k, u in enumerate(units) if u[3] != (1.0, 1.0, 1.0)]
        assert all(k in der for k in E.EDGE_UNITS if k < ngen)
        if ngen >= 8:                                                                 # every kind of hl1_ms_kinds in every state
            kinds = {(s, 1 if units[k][3][s] >= 1.0 else 0 if units[k][3][s] <= 0.0 else 2) for k in der for s in range(3)}
            assert kinds == {(s, q) for s in range(3) for q in range(3)}, (ngen, kinds)
    assert E.MS_NHOURS_EDGES == (1, 24, 63, 64, 65, 255, 256, 257, 511, 512, 513) and MM.WINDOW == 256


def test_area_var_max_case_is_the_largest_configuration():
    for H in (48, 513):
        c = E.area_var_max_case(H)
        assert len(c["units"]) == 8 and sum(c["units"]) == 128 and len(c["ties"]) == 32 and c["loads"].shape == (8, H)
        assert np.all(np.isfinite(c["tie_mttf"])) and np.all(np.isfinite(c["tie_mttr"])) and c["tie_mttr"].min() < 0.3 and c["tie_mttf"].min() < 6.0
        assert len(c["resource_area"]) == 8 and {0, 7} <= set(c["resource_area"]) and c["resource_scale"].count(0.0) == 1
        assert len(c["storages"]) == 8 and {0, 7} <= {a for a, _ in c["storages"]}
        assert c["out"].shape == (3, 8, H) and c["wl"].shape == (3, 8, H) and not c["out"][1, 7].any()
    # the dynamic LDS of the largest call, as csrc/relmc_area_variable.hip sizes it: rows of 64 doubles, then 4 + 1 mask rows of 512 words
    rows = (8 + 1) + (2 * (8 + 1) + 8) + 8 + 8 * 8
    assert rows == 107 and rows * 512 + 5 * 512 * 4 == 65024 <= 65536


# ---- the models against the literal loops ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", LITERAL)
def test_weather_model_equals_the_literal_hour_loops(label):
    """variable_model on the edge library (3 weather years with curves, 3 resources, edge_storages) against
    hl1_variable_model.literal_variable_chain, every number of every year bit for bit (both sum a year in step order); and with every
    resource scaled 0 and no curves against hl1_storage_model.literal_storage_chain, the loop tests/test_hl1_chrono_edges_host.py uses:
    the host form of the device test's first pin."""
    _, (cap, mttf, mttr, load), seed, first, n, years, start, pick = _shape(label)
    out, wl, st, rec, W, _ = _weather_case(label)
    chains = _middle(first)
    lit = [VM.literal_variable_chain(seed, c, cap, mttf, mttr, load, years, start, out, wl, RS3, pick, st) for c in chains]
    np.testing.assert_array_equal(rec[2 * years:6 * years], np.concatenate([x[0] for x in lit]))
    np.testing.assert_array_equal(W[2 * years:6 * years], np.concatenate([x[1] for x in lit]))
    rec = rec[2 * years:6 * years]
    zero, _ = VM.variable_model(seed, chains, cap, mttf, mttr, load, years, start, out, None, (0.0, 0.0, 0.0), pick, st)
    np.testing.assert_array_equal(zero, np.concatenate([SM.literal_storage_chain(seed, c, cap, mttf, mttr, load, years, start, st) for c in chains]))
    assert zero.tobytes() != rec.tobytes()


@pytest.mark.parametrize("label", LITERAL)
def test_stress_model_equals_the_literal_hour_loop(label):
    """stress_model on edge_stress and edge_classes against literal_stress_chain, which spends the draws on the multipliers themselves
    and has no storages: loss hours and events of every year exact, EUE to 1e-12 (tests/test_hl1_stress_host.py's rule).  The spikes are
    2^10 here, not edge_stress's 2^60: every unit still fails within the hour of its repair (counted), but no draw is absorbed, so no
    failure is rounded onto a whole hour, where the contract's step rule and a loop in real arithmetic part by one step (edge_stress)."""
    _, (cap, mttf, mttr, load), seed, first, n, years, start, pick = _shape(label)
    out, wl, _, _, cls = _stress_case(label)[:5]
    mult = E.edge_stress(3, 3, len(load), spike=2.0 ** 10)
    chains = _middle(first)
    cnt = {}
    rec, W = XM.stress_model(seed, chains, cap, mttf, mttr, load, years, start, out, mult, cls, wl, RS3, pick, counters=cnt)
    assert cnt["immediate"] > 0 and cnt["carried"] > 0 and cnt["flat"] == 0 and 0 < cnt["never"] < cnt["failures"], cnt
    lit = [XM.literal_stress_chain(seed, c, cap, mttf, mttr, load, years, start, out, mult, cls, wl, RS3, pick) for c in chains]
    got = np.concatenate([x[0] for x in lit])
    np.testing.assert_array_equal(rec[:, [0, 2]], got[:, [0, 2]])
    np.testing.assert_allclose(rec[:, 1], got[:, 1], rtol=1e-12)
    np.testing.assert_array_equal(W, np.concatenate([x[1] for x in lit]))
    assert rec[:, 0].sum() > 0


MS_LITERAL = ("h1-0", "h64-1", "h65-0", "h255-1", "h256-0", "h257-1", "h513-1", "g1-1", "g65-0", "g128-1")


@pytest.mark.parametrize("label", MS_LITERAL)
def test_multistate_model_equals_the_literal_hour_loop(label):
    """interval_model against literal_chain on ms_fleet: every count exact, EUE as tests/test_hl1_multistate_host.py compares it."""
    _, fleet, seed, first, n, years, start = MS_SHAPES[MS_IDS.index(label)]
    units, _, load = E.ms_fleet(*fleet)
    chains = _middle(first)
    a = MM.interval_model(seed, chains, units, load, years, start)
    b = np.concatenate([MM.literal_chain(seed, c, units, load, years, start) for c in chains])
    np.testing.assert_array_equal(a[:, [0, 2, 3, 4]], b[:, [0, 2, 3, 4]])
    np.testing.assert_allclose(a[:, 1], b[:, 1], rtol=1e-12, atol=1e-9)
    assert a[:, 0].sum() > 0 and a[:, 3].sum() > 0 and a[:, 4].sum() > 0


# ---- the paths the shapes reach ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", IDS)
def test_weather_shapes_reach_every_path(label):
    """track_coverage on the weather case of every shape: short, lost and discharging steps, quiet and serial groups and all three
    weather years everywhere; long, served and charging steps on every year longer than an hour (storage_coverage's exemption of
    nhours = 1, by that name); two weather years inside one 64-step group on every year shorter than a group."""
    _, (cap, mttf, mttr, load), seed, first, n, years, start, pick = _shape(label)
    _, _, _, rec, W, cnt = _weather_case(label)
    E.track_coverage(label, cnt, W, len(load), years)
    assert cnt["long"] > 0 and sum(cnt["charge"]) > 0                 # edge_weather gives nhours = 1 surplus hours too


@pytest.mark.parametrize("label", IDS)
def test_stress_shapes_reach_every_path(label):
    """track_coverage and stress_coverage on the stress case of every shape; the named exemptions are stress_coverage's: nhours = 1 has no
    landing on an hour without slope, a one-unit fleet no failure of a class -1 unit."""
    _, (cap, mttf, mttr, load), seed, first, n, years, start, pick = _shape(label)
    rec, W, cnt, steps = _stress_case(label)[5:]
    E.track_coverage(label, steps, W, len(load), years)
    E.stress_coverage(label, cnt, len(load), len(cap))
    assert rec.tobytes() != _weather_case(label)[3].tobytes()          # the stress is felt


@pytest.mark.parametrize("shape", MS_SHAPES, ids=MS_IDS)
def test_multistate_shapes_reach_every_path(shape):
    label, fleet, seed, first, n, years, start = shape
    units, _, load = E.ms_fleet(*fleet)
    E.ms_coverage(label, fleet[1], MM.path_counts(seed, range(first, first + n), units, load, years, start))


def test_all_256_weather_years_occur():
    """The n_weather = 256 case of the device test: H = 24, 48 chains of 67 years under either pick."""
    cap, mttf, mttr, load = E.seq_fleet(8, 24)
    years = E.seq_years(24)
    for pick in (VM.PICK_RANDOM, VM.PICK_CYCLE):
        assert np.unique(VM.weather_years(13, range(40, 88), years, 256, pick)).size == 256


# ---- a subtly wrong kernel would fail ---------------------------------------------------------------------------------------------------------
def _perturbed(kind):
    """-> (records of the case, records of the model with one subtle fault) on the case the device test compares."""
    if kind.endswith("upper-word") and kind != "chain-upper-word":
        label = "g65-1"                                               # first_chain = 2^32 - 4: chains 2^32 .. 2^32 + 3 are in it
        _, (cap, mttf, mttr, load), seed, first, n, years, start, _ = _shape(label)
        pick, nw = E.UPPER_WORD_PICKS[0 if "random" in kind else 1]
        chains = np.arange(first, first + n, dtype=np.uint64)
        assert int(chains[-1]) >> 32 == 1
        low = VM.weather_years(seed, chains & np.uint64(0xFFFFFFFF), years, nw, pick).reshape(n, years)
        true = VM.weather_years(seed, chains, years, nw, pick)
        for j in range(4):                                            # chain 2^32 + j and chain j differ in their weather
            assert not np.array_equal(true[4 + j], low[4 + j]), j
        if kind.startswith("weather"):
            out, wl, st, rec, W, _ = _weather_case(label, pick, nw)
            bad, _ = VM.variable_model(seed, chains, cap, mttf, mttr, load, years, start, out, wl, RS3, pick, st, weather=low)
        else:
            out, wl, st, mult, cls, rec, W = _stress_case(label, pick, nw)[:7]
            bad, _ = XM.stress_model(seed, chains, cap, mttf, mttr, load, years, start, out, mult, cls, wl, RS3, pick, st, weather=low)
        for j in range(4):                                            # and in their records, chain by chain
            s = slice((4 + j) * years, (5 + j) * years)
            assert bad[s].tobytes() != rec[s].tobytes(), j
        assert bad[:4 * years].tobytes() == rec[:4 * years].tobytes()
        return rec, bad
    if kind == "chain-upper-word":                                    # the whole chain index without its upper word: other draws, other records
        label = "g65-1"
        _, (cap, mttf, mttr, load), seed, first, n, years, start, pick = _shape(label)
        out, wl, st, rec, W, _ = _weather_case(label)
        bad, _ = VM.variable_model(seed, range(4), cap, mttf, mttr, load, years, start, out, wl, RS3, pick, st)
        return rec[4 * years:], bad
    if kind == "odd-tail-resource":
        label = "h65-0"
        _, (cap, mttf, mttr, load), seed, first, n, years, start, pick = _shape(label)
        out, wl, st, rec, W, _ = _weather_case(label)
        bad, _ = VM.variable_model(seed, range(first, first + n), cap, mttf, mttr, load, years, start, out, wl, RS3[:2] + (0.0,), pick, st)
        return rec, bad
    if kind in ("class-of-slot-0-g65", "class-of-slot-0-g128"):
        label = "g65-0" if kind.endswith("g65") else "g128-1"
        _, (cap, mttf, mttr, load), seed, first, n, years, start, pick = _shape(label)
        out, wl, st, mult, cls, rec, W = _stress_case(label)[:7]
        wrong = cls.copy()
        wrong[64:] = cls[:len(cls) - 64]
        assert not np.array_equal(wrong, cls)
        bad, _ = XM.stress_model(seed, range(first, first + n), cap, mttf, mttr, load, years, start, out, mult, wrong, wl, RS3, pick, st)
        return rec, bad
    raise KeyError(kind)


@pytest.mark.parametrize("kind", ["weather-random-upper-word", "weather-cycle-upper-word", "stress-random-upper-word", "stress-cycle-upper-word", "chain-upper-word", "odd-tail-resource", "class-of-slot-0-g65",
                                  "class-of-slot-0-g128"])
def test_a_subtly_wrong_model_gives_other_records(kind):
    """What the device is compared with changes when the model is given one fault a kernel could have: the weather pick without the
    chain's upper word (chain 2^32 + j then has chain j's weather years; under the picks of UPPER_WORD_PICKS, since CYCLE over three
    weather years in six-year chains gives both chains the same years), the chain without it altogether, the third resource (the odd
    tail of the resource loop) left out, the class of unit k read for unit k + 64 (the lane's second slot).  Counts differ, not only
    energies: the device test's exact comparisons would fail."""
    rec, bad = _perturbed(kind)
    assert rec.shape == bad.shape and not np.array_equal(rec[:, [0, 2, 3]], bad[:, [0, 2, 3]])


def test_area_weather_cases_reach_their_paths():
    """The 4-area tie-edge case of the device test at its shortest and longest year, from the area model's counters: transfers, storages
    that charge and discharge, an import followed by a storage, quiet and serial groups (nhours = 1: a chain of 1600 one-hour years has
    a short step in every group, so no quiet group; it is exempt as it is from the surplus conditions)."""
    for H in (1, 513):
        c = E.area_var_tie_case(65, H)
        years = E.seq_years(H)
        for first in (0, (1 << 32) - 2):
            cnt = AVM.new_counters(4)
            rec, W = AVM.area_variable_model(17, range(first, first + 4), c["units"], c["cap"], c["mttf"], c["mttr"], c["loads"], c["ties"], years,
                                             AVM.STATIONARY, AVM.INTERCONNECTED, AVM.MAX_FLOW, c["out"], c["resource_area"], c["wl"],
                                             c["resource_scale"], storages=c["storages"], tie_mttf=c["tie_mttf"], tie_mttr=c["tie_mttr"], counters=cnt)
            assert cnt["transfer_steps"] > 0 and cnt["serial_groups"] > 0 and rec[:, 4, 0].sum() > 0, (H, cnt)
            assert sum(cnt["discharge"]) > 0 and cnt["served"][4] > 0, (H, cnt)
            if H > 1:
                assert cnt["quiet_groups"] > 0 and sum(cnt["charge"]) > 0, (H, cnt)
            assert np.unique(W).size == 3
