"""The host side of tests/test_hl1_chrono_edges.py (no GPU): the storage model against a literal hour loop of the contract
(hl1_storage_model.literal_storage_chain) on every shape the device test runs, the lane-edge pattern worked out by hand on both, and the
paths the shapes reach, read off the models alone: a shape that stops exercising a path fails here, before any GPU run."""
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


E, SM, EV = (_tool(n) for n in ("hl1_edge_cases", "hl1_storage_model", "hl1_event_model"))
SEQ = SM.SEQ
SHAPES = E.chrono_shapes()
IDS = [s[0] for s in SHAPES]
# tests/test_hl1_storage.py's eight unlike storages: one that cannot charge, one that cannot discharge, one without energy
EIGHT = [(20.0, 5.0, 10.0, 0.9, 0.95, 10.0), (3.0, 4.0, 8.0, 1.0, 1.0, 0.0), (10.0, 6.0, 30.0, 0.85, 0.8, 15.0), (0.0, 7.0, 20.0, 1.0, 0.9, 20.0),
         (5.0, 0.0, 10.0, 0.9, 0.9, 5.0), (2.0, 3.0, 0.0, 0.7, 0.7, 0.0), (6.0, 8.0, 24.0, 0.95, 0.95, 24.0), (50.0, 50.0, 12.5, 0.5, 0.5, 0.0)]


def _same(model, literal):
    """Counts exact and the three energies bit for bit: storage_chain and the literal loop both sum a year in step order."""
    np.testing.assert_array_equal(model, literal)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_storage_model_equals_the_literal_hour_loop(shape):
    """storage_model (the interval form's capacities, storage_chain's step rule) against literal_storage_chain (the reference's hour loop
    for the units, the contract's text for the storages) on every chain of every shape, with edge_storages: all six numbers of every
    year are equal bit for bit (both sum a year in step order).  The model's counters satisfy the coverage conditions, and the literal
    loop counts the same steps."""
    label, (cap, mttf, mttr, load), seed, first, n, years, start = shape
    st = E.edge_storages(cap)
    rec, cnt = SM.storage_model(seed, range(first, first + n), cap, mttf, mttr, load, years, start, st)
    lit_cnt = {}
    lit = np.concatenate([SM.literal_storage_chain(seed, c, cap, mttf, mttr, load, years, start, st, counters=lit_cnt)
                          for c in range(first, first + n)])
    _same(rec, lit)
    E.storage_coverage(label, cnt)
    for key in ("short", "long", "served", "lost"):
        assert cnt[key] == lit_cnt[key], key
    assert cnt["discharge"] == lit_cnt["discharge"] and cnt["charge"] == lit_cnt["charge"]


@pytest.mark.parametrize("start", [SEQ.ALL_UP, SEQ.STATIONARY])
def test_storage_model_equals_the_literal_hour_loop_with_eight_storages(start):
    """The small fleet with tests/test_hl1_storage.py's eight storages, at a raised level (scale and shift are part of the loop)."""
    cap, mttf, mttr, load = SEQ.small_fleet()
    for scale, shift in ((1.0, 0.0), (1.07, 3.25)):
        rec, cnt = SM.storage_model(7, range(8), cap, mttf, mttr, load, 3, start, EIGHT, scale, shift)
        lit = np.concatenate([SM.literal_storage_chain(7, c, cap, mttf, mttr, load, 3, start, EIGHT, scale, shift) for c in range(8)])
        _same(rec, lit)
        assert cnt["served"] > 0 and cnt["lost"] > 0 and all(cnt["discharge"][i] > 0 for i in (0, 1, 2, 3, 6, 7))


def test_lane_edge_pattern_on_the_model_and_the_literal_loop():
    """The six numbers per year derived in lane_edge_pattern's docstring, on storage_chain (with its trace: the storage is exactly full
    before each run, empty after it, and at 30 then 32 MWh on the tenth and eleventh hour of a refill) and on the literal loop."""
    curve, storage, years, want = SM.lane_edge_pattern()
    H = len(curve)
    assert H == 130 and years == 3
    trace = []
    rec, final = SM.storage_chain([100.0] * (years * H), curve, years, [storage], trace=trace)
    np.testing.assert_array_equal(rec, want)
    assert final == [0.0]
    soc = [t[0][0] for t in trace]
    deficit = [t[1] for t in trace]
    for y in range(years):
        o = y * H
        assert soc[o + 61] == 32.0 and soc[o + 62:o + 65] == [24.0, 0.0, 0.0] and deficit[o + 62:o + 65] == [0.0, 4.0, 8.0]
        assert soc[o + 65:o + 77] == [3.0 * k for k in range(1, 11)] + [32.0, 32.0] and soc[o + 126] == 32.0
        assert soc[o + 127:o + 130] == [20.0, 0.0, 0.0] and deficit[o + 127:o + 130] == [0.0, 2.0, 2.0]
        assert sum(deficit[o:o + H]) == 16.0
    # where the short steps sit in the device's 64-step groups: lane 63 and lane 0 of adjacent groups, and the six-step last group
    short = [y * H + h for y in range(years) for h in (62, 63, 64, 127, 128, 129)]
    assert [q % 64 for q in short[:6]] == [62, 63, 0, 63, 0, 1] and [q % 64 for q in short[6:12]] == [0, 1, 2, 1, 2, 3]
    assert short[-3:] == [387, 388, 389] and years * H - 384 == 6
    lit = SM.literal_storage_chain(3, 0, [100.0], [1e15], [1.0], curve, years, SEQ.ALL_UP, [storage])
    np.testing.assert_array_equal(lit, want)
    none = SM.literal_storage_chain(3, 0, [100.0], [1e15], [1.0], curve, years, SEQ.ALL_UP, [])
    np.testing.assert_array_equal(none, np.tile([6.0, 48.0, 2.0, 0.0, 0.0, 0.0], (3, 1)))


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_event_shapes_hold_every_edge_kind(shape):
    label, (cap, mttf, mttr, load), seed, first, n, years, start = shape
    ev = EV.interval_events(seed, range(first, first + n), cap, mttf, mttr, load, years, start)
    k = EV.kinds(ev, len(load), years)
    E.event_coverage(label, len(load), k)
    per_chain = np.bincount(ev["chain"], minlength=n)
    assert 0 < per_chain[:3].sum() < k["n"] - 1                 # the two short buffers of the device test end inside the list


def test_edge_levels_and_withheld_units():
    """edge_levels(n) is a prefix of edge_levels(16); from five levels on it holds the identity, both extremes and two fleet-1 levels.
    The withheld units lie in the first and in the last mask word of the fleet."""
    full = E.edge_levels(16)
    assert len(set(full)) == 16 and full[0] == (1.0, 0.0, 0)
    for n in (1, 2, 4, 5, 8, 9, 16):
        lv = E.edge_levels(n)
        assert lv == full[:n]
        if n >= 5:
            assert E.NEVER_LOSES in lv and E.ALWAYS_LOSES in lv and sum(f for _, _, f in lv) >= 2
    assert sum(1 for s, t, f in full if f == 0 and (s, t) != (1.0, 0.0)) >= 8
    for ngen in E.NGEN_EDGES + (8,):
        wh = E.edge_withheld(ngen)
        assert wh[0] == 0 and wh[-1] == ngen - 1 and {k >> 5 for k in wh} == {0, (ngen - 1) >> 5}
    cap, mttf, mttr, load = E.seq_fleet(128, 100)
    assert load.max() < 1e9 and 0.0 <= cap.min()                # the extremes are extremes: 0 <= cap_avail < 1e9, and -1 is below it
