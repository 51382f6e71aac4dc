"""Cases at the edges of the HL1 contracts (include/relmc.h), shared by tests/test_hl1_edges.py (device against the host models) and
tests/test_hl1_edges_host.py (host models against the reference loops): unit counts around the 4-unit Philox blocks, the 32-bit mask words
and the two lanes' slots, years shorter than a 64-lane group or straddling the 512-step window, transitions far shorter than a step or far
longer than the horizon, zero capacities, loads equal to reachable capacity sums, 8 areas on the topologies where augmenting paths are
long, 32 failing ties on years around the window length, and the planning model's 8 ELU slots in week 53.  tests/test_hl1_chrono_edges.py
and its _host companion run the sweep, storage and event kernels on the same seq shapes (chrono_shapes), with the storages, sweep levels,
withheld units and coverage conditions defined beside them.  Every value is computed here; nothing is read from disk."""
from __future__ import annotations

import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle.pyoracle import philox4x32_10  # noqa: E402

FOR_EXTREMES = (0.0, 2.0 ** -32, 0.5, 1.0 - 2.0 ** -32, 1.0)
RECORD_BUDGET = 1 << 22              # kHl1RecordBudget (csrc/relmc_hl1_host.h): the year records a launch of the chain models holds at most


def unit_order_sum(cap, up):
    """Sum of cap[k] over the up units in ascending unit order (the kernels' order), one value per row of up[rows, K]."""
    s = np.zeros(up.shape[0])
    for k in range(len(cap)):
        s = s + np.where(up[:, k], float(cap[k]), 0.0)
    return s


# ---- relmc_hl1_nsq ---------------------------------------------------------------------------------------------------------------
def nsq_thresholds(for_rate):
    """The clamped contract: thr = floor(for_rate * 2^32) clamped to [0, 2^32 - 1]."""
    t = np.floor(np.asarray(for_rate, dtype=np.float64) * 4294967296.0)
    return np.clip(np.where(t > 0, t, 0.0), 0.0, 4294967295.0).astype(np.uint64)


def nsq_up(seed, first_index, n, for_rate):
    """up[i, g] of iteration first_index + i: draw word g & 3 of philox(ctr = (i_lo, i_hi, g >> 2, 0), key = seed) >= thr_g."""
    K = len(for_rate)
    nb = (K + 3) // 4
    gi = np.uint64(first_index) + np.arange(n, dtype=np.uint64)
    ctr = np.zeros((n, nb, 4), dtype=np.uint32)
    ctr[..., 0] = (gi & np.uint64(0xFFFFFFFF)).astype(np.uint32)[:, None]
    ctr[..., 1] = (gi >> np.uint64(32)).astype(np.uint32)[:, None]
    ctr[..., 2] = np.arange(nb, dtype=np.uint32)[None, :]
    key = np.zeros((n, nb, 2), dtype=np.uint32)
    key[..., 0] = np.uint32(seed & 0xFFFFFFFF)
    key[..., 1] = np.uint32(seed >> 32)
    w = philox4x32_10(ctr, key).reshape(n, nb * 4)[:, :K].astype(np.uint64)
    return w >= nsq_thresholds(for_rate)[None, :]


def nsq_fleet(ngen):
    """ngen units with non-integer capacities; the five FOR extremes cycle through units 0..4, the other units have FOR 0.02 .. 0.3."""
    rng = np.random.default_rng(1000 + ngen)
    cap = np.round(rng.uniform(5.0, 80.0, ngen), 3) + 0.0625
    forr = rng.uniform(0.02, 0.3, ngen)
    forr[:min(ngen, 5)] = FOR_EXTREMES[:min(ngen, 5)]
    return cap, forr


def nsq_load(cap, forr, nhours, ties=()):
    """nhours loads spread over the fleet's likely available capacity; the values in `ties` replace the first hours (exact ties)."""
    rng = np.random.default_rng(nhours + 7 * len(cap))
    mean = float((np.asarray(cap) * (1.0 - np.asarray(forr))).sum())
    sd = math.sqrt(float((np.asarray(cap) ** 2 * np.asarray(forr) * (1.0 - np.asarray(forr))).sum())) + 1.0
    load = mean + sd * rng.uniform(-1.5, 3.0, nhours)
    t = np.asarray(ties, dtype=np.float64)[:nhours]
    load[:t.size] = t
    return load


def eue_scales():
    """(label, base, spread): flat curves base + U(0, spread) just above a fleet whose all-up capacity is exactly `base`."""
    return (("1000+U(0,1e-3)", 1000.0, 1e-3), ("3000+U(0,1e-6)", 3000.0, 1e-6), ("1e5+U(0,1e-3)", 1e5, 1e-3))


def eue_case(base, spread, nhours=8760):
    """4 units summing to `base` exactly in unit order (FOR 0.01: most iterations are all up) and the flat curve above it."""
    cap = np.array([0.375, 0.25, 0.125, 0.25]) * base
    assert cap[0] + cap[1] + cap[2] + cap[3] == base
    forr = np.full(4, 0.01)
    load = base + np.random.default_rng(int(base) + 3).uniform(0.0, spread, nhours)
    return cap, forr, load


def exact_eue(caps, load):
    """math.fsum of the per-hour deficits of every iteration (a deficit load - cap of a flat curve is exact by Sterbenz)."""
    srt = np.sort(np.asarray(load, dtype=np.float64))
    uniq, inv = np.unique(np.asarray(caps, dtype=np.float64), return_inverse=True)
    return np.array([math.fsum((srt[srt > c] - c).tolist()) for c in uniq])[inv]


# ---- relmc_hl1_seq ---------------------------------------------------------------------------------------------------------------
def seq_fleet(ngen, nhours, seed=0):
    """ngen units with non-integer capacities, a zero-capacity unit, units with MTTR << 1 h (several transitions inside one step, empty
    intervals) and units with MTTF >> any horizon (no transition); the load curve straddles the mean available capacity and its first
    hours equal reachable capacity sums (all up; all up but unit j), summed in unit order."""
    rng = np.random.default_rng(50 + ngen + 1000 * seed)
    cap = np.round(rng.uniform(5.0, 60.0, ngen), 3) + 0.125
    mttf = rng.uniform(20.0, 300.0, ngen)
    mttr = rng.uniform(2.0, 40.0, ngen)
    if ngen > 1:
        cap[1] = 0.0
    mttr[2::5] = rng.uniform(0.01, 0.3, mttr[2::5].size)
    mttf[2::10] = rng.uniform(1.0, 3.0, mttf[2::10].size)
    mttf[3::7] = 1e12
    h = np.arange(nhours)
    q = mttr / (mttf + mttr)
    avail = float((cap * (1.0 - q)).sum())
    sd = math.sqrt(float((cap ** 2 * q * (1.0 - q)).sum())) + 0.5
    load = avail + sd * (0.3 + 1.2 * np.sin(2 * np.pi * h / 24.0 + 0.3) + 0.4 * np.cos(2 * np.pi * h / max(nhours, 2)))
    up = np.ones((1 + min(ngen, 4), ngen), dtype=bool)
    for j in range(1, up.shape[0]):
        up[j, j - 1] = False
    ties = unit_order_sum(cap, up)
    load[:min(nhours, ties.size)] = ties[:nhours]
    if nhours > 8:
        load[nhours // 2] = ties[0]
    return cap, mttf, mttr, load


def seq_years(nhours, steps=1600):
    """Years per chain so that a chain runs about `steps` steps (several 512-step windows), at least 2."""
    return max(2, -(-steps // nhours))


NHOURS_EDGES = (1, 24, 63, 64, 65, 511, 512, 513)                # year lengths of the seq edge tests: below, at and around a group and a window
NGEN_EDGES = (1, 32, 33, 64, 65, 128)                            # unit counts of the seq edge tests: mask words and lane slots full and one over


def chrono_shapes():
    """The shapes of the seq edge tests as (label, fleet, seed, first_chain, n_chains, years, start), start 0 = all UP, 1 = stationary:
    seq_fleet(8, nhours) on chains 40 .. 47 under both start rules, and seq_fleet(ngen, 100), 6 years, all UP from chain 0 and stationary
    across first_chain = 2^32."""
    out = []
    for nhours in NHOURS_EDGES:
        for start in (0, 1):
            out.append(("h%d-%d" % (nhours, start), seq_fleet(8, nhours), 13, 40, 8, seq_years(nhours), start))
    for ngen in NGEN_EDGES:
        for start, first in ((0, 0), (1, (1 << 32) - 4)):
            out.append(("g%d-%d" % (ngen, start), seq_fleet(ngen, 100), 3, first, 8, 6, start))
    return out


def edge_storages(cap):
    """Three storages (charge_mw, discharge_mw, energy_mwh, eta_charge, eta_discharge, soc0_mwh) as fractions of the installed capacity:
    a lossy one that starts full, a small one that starts empty and discharges without loss, and a large slow one (it charges at 5 % and
    delivers 0.4 % of the fleet an hour) that starts half full and charges without loss."""
    tot = float(np.sum(np.asarray(cap, dtype=np.float64)))
    return [(0.02 * tot, 0.03 * tot, 0.08 * tot, 0.9, 0.95, 0.08 * tot),
            (0.01 * tot, 0.015 * tot, 0.02 * tot, 0.85, 1.0, 0.0),
            (0.05 * tot, 0.004 * tot, 0.5 * tot, 1.0, 0.8, 0.5 * (0.5 * tot))]


def storage_coverage(label, cnt):
    """The conditions on a shape's inputs under edge_storages, on hl1_storage_model's counters: some short step is lost although the
    first storage delivers; on every year longer than an hour some step is long, some short step is served in full and some storage
    charges.  nhours = 1 is a flat curve without a surplus hour, so the three surplus conditions do not apply to it."""
    assert cnt["short"] > 0 and cnt["lost"] > 0 and cnt["discharge"][0] > 0, (label, cnt)
    if not label.startswith("h1-"):
        assert cnt["long"] > 0 and cnt["served"] > 0 and sum(cnt["charge"]) > 0, (label, cnt)


def event_coverage(label, nhours, kinds):
    """The conditions on a shape's events, on hl1_event_model.kinds' counts: with a year of 63 hours or more some event crosses a
    64-step group edge, one a 512-step window edge and one a year boundary."""
    assert kinds["n"] > 0, (label, kinds)
    if nhours >= 63:
        assert kinds["edge64"] >= 1 and kinds["edge512"] >= 1 and kinds["year"] >= 1, (label, kinds)


NEVER_LOSES, ALWAYS_LOSES =(0.0, -1.0, 0), (0.0, 1e9, 0)        # L = -1 is below every capacity sum, L = 1e9 above every one
_SPREAD = [(0.9, 0.0, 0), (1.12, -0.5, 0), (0.85, 2.75, 1), (0.95, 1.5, 0), (0.65, 0.0, 1), (1.03, -1.25, 0), (0.85, 4.0, 0), (1.2, 0.0, 0),
           (0.9, 0.0, 1), (1.0, -3.5, 0), (1.16, 0.25, 0)]


def edge_levels(n):
    """n sweep levels (scale, shift, fleet), 1 <= n <= 16: the identity, a level on fleet 1 at the loaded curve, one that never loses,
    one that always loses, a lowered level on fleet 1, then levels of both fleets spread between the extremes (scales 0.65 .. 1.2, dyadic
    shifts of a few MW; the fleet-1 levels are lowered by different amounts, since two withheld units of eight weigh more than four of
    128).  Every n >= 5 holds the first five; a shorter list is a prefix, so level j is the same level at every n."""
    levels = [(1.0, 0.0, 0), (1.0, 0.0, 1), NEVER_LOSES, ALWAYS_LOSES, (0.75, 0.75, 1)] + _SPREAD
    assert 1 <= n <= len(levels) == 16
    return levels[:n]


def edge_withheld(ngen):
    """The withheld units of the fleet-1 levels: the first and the last unit of the first and of the last mask word the fleet has (at
    128 units: both lane slots, words 0 and 3)."""
    last = 32 * ((ngen - 1) // 32)
    return sorted({0, min(31, ngen - 1), last, ngen - 1})


# ---- relmc_hl1_area --------------------------------------------------------------------------------------------------------------
UNITS8 = [1, 1, 30, 40, 20, 10, 25, 1]                          # 128 units, uneven, three single-unit areas


def area_fleet8(nhours=48, seed=0):
    """128 units in 8 areas (UNITS8, area-major), non-integer capacities, fast repair on some units; loads per area near each area's
    mean available capacity, area 0 in surplus and area 7 short (the path topology's 7-hop transfers)."""
    rng = np.random.default_rng(77 + seed)
    K = sum(UNITS8)
    cap = np.round(rng.uniform(5.0, 50.0, K), 3) + 0.25
    mttf = rng.uniform(40.0, 400.0, K)
    mttr = rng.uniform(3.0, 50.0, K)
    mttr[5::9] = rng.uniform(0.02, 0.4, mttr[5::9].size)
    lo = np.concatenate([[0], np.cumsum(UNITS8)])
    h = np.arange(nhours)
    loads = np.zeros((8, nhours))
    for a in range(8):
        s = slice(lo[a], lo[a + 1])
        avail = float((cap[s] * mttf[s] / (mttf[s] + mttr[s])).sum())
        level = 0.6 if a == 0 else (1.08 if a == 7 else 0.95)
        loads[a] = avail * (level + 0.08 * np.sin(2 * np.pi * (h - 3 * a) / 24.0))
    return list(UNITS8), cap, mttf, mttr, loads


def topologies8():
    """name -> ties [(from, to, capacity)] on 8 areas."""
    rng = np.random.default_rng(5)
    complete = [(i, j, float(np.round(rng.uniform(5.0, 40.0), 2))) for i in range(8) for j in range(i + 1, 8)]
    complete += [(j, i, 7.5) for i, j, _ in complete[::4]]                                # parallel ties, reversed endpoints
    return {
        "complete": complete,
        "path": [(i, i + 1, 60.0 + 5.0 * i) for i in range(7)],
        "star": [(0, j, 30.0 + 4.0 * j) for j in range(1, 8)],
        "two_components": [(0, 1, 25.0), (1, 2, 35.5), (2, 3, 20.0), (0, 3, 10.0), (4, 5, 40.0), (5, 6, 15.25), (6, 7, 30.0), (4, 7, 12.0)],
        "zero_ties": [(i, i + 1, 0.0) for i in range(7)] + [(0, 7, 0.0)],
    }


def area_tie_edges(ngen, nhours):
    """The tie slot of the chronology at its edges: seq_fleet(ngen) split over 4 areas (the second has one unit), a year of nhours hours
    and 32 ties on the 6 area pairs (every tie lane busy; parallel ties, every second one with its endpoints reversed): some with
    MTTR << 1 h (several transitions inside one step, empty intervals), some with an MTTF of a few hours, tie 7 with mttf = inf (no
    cursor) and tie 12 with mttf = 1e30 (a T without an int64 image).  Area loads near each area's mean available capacity, so that the
    small tie capacities decide about loss hours.  -> units, cap, mttf, mttr, loads[4][nhours], ties [(from, to, capacity)], kf, kr."""
    cap, mttf, mttr, _ = seq_fleet(ngen, nhours)
    units = [20, 1, 25, ngen - 46]
    lo = np.concatenate([[0], np.cumsum(units)])
    h = np.arange(nhours)
    loads = np.zeros((4, nhours))
    for a, level in enumerate((0.6, 0.7, 0.8, 0.85)):
        s = slice(lo[a], lo[a + 1])
        avail = float((cap[s] * mttf[s] / (mttf[s] + mttr[s])).sum())
        loads[a] = avail * (level + 0.1 * np.sin(2 * np.pi * (h - 5 * a) / 24.0))
    rng = np.random.default_rng(900 + ngen)
    pairs = [(i, j) for i in range(4) for j in range(i + 1, 4)]
    tcap = np.round(rng.uniform(1.0, 6.0, 32), 2)
    ties = [pairs[t % 6][::-1 if t % 2 else 1] + (float(tcap[t]),) for t in range(32)]
    kf = rng.uniform(30.0, 200.0, 32)
    kr = rng.uniform(3.0, 30.0, 32)
    kr[2::5] = rng.uniform(0.01, 0.3, kr[2::5].size)
    kf[1::6] = rng.uniform(2.0, 6.0, kf[1::6].size)
    kf[7], kf[12] = math.inf, 1e30
    return units, cap, mttf, mttr, loads, ties, kf, kr


# ---- relmc_hl1_plan --------------------------------------------------------------------------------------------------------------
def plan_fleet(ngen, nhours=8760, n_elu=0, binding=True, sigma_frac=0.03):
    """ngen units with non-integer capacities, FOR 0.02 .. 0.15, maintenance windows that run past the end of the year or start in
    week 53 (when nhours reaches it), the last n_elu units energy-limited (small limits when binding, finite but never reached
    otherwise), a load curve near the mean available capacity; -> (cap, forr, start, weeks, limit, load), sigma."""
    rng = np.random.default_rng(300 + ngen + 17 * n_elu + (0 if binding else 1))
    cap = np.round(rng.uniform(10.0, 90.0, ngen), 3) + 0.137
    forr = rng.uniform(0.02, 0.15, ngen)
    start = np.zeros(ngen, dtype=np.int32)
    weeks = np.zeros(ngen, dtype=np.int32)
    windows = [(52, 3), (53, 1), (53, 5), (1, 2), (51, 2)]
    for k in [k for k in range(ngen) if k < 3 or k % 3 == 0]:
        start[k], weeks[k] = windows[k if k < 3 else (k // 3) % len(windows)]
    limit = np.full(ngen, math.inf)
    if n_elu:
        elu = np.arange(ngen - n_elu, ngen)
        limit[elu] = cap[elu] * (rng.uniform(20.0, 60.0, n_elu) if binding else 1e9)
    h = np.arange(nhours)
    avail = float((cap * (1.0 - forr)).sum())
    load = avail * (0.8 + 0.12 * np.sin(2 * np.pi * h / 24.0) + 0.05 * np.sin(2 * np.pi * h / 8760.0 * 3))
    return (cap, forr, start, weeks, limit, load), sigma_frac * avail
