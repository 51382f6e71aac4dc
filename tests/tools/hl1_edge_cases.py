"""Cases at the edges of the HL1 contracts (include/relmc.h), shared by tests/test_hl1_edges.py (device against the host models) and
tests/test_hl1_edges_host.py (host models against the reference loops): unit counts around the 4-unit Philox blocks, the 32-bit mask words
and the two lanes' slots, years shorter than a 64-lane group or straddling the 512-step window, transitions far shorter than a step or far
longer than the horizon, zero capacities, loads equal to reachable capacity sums, 8 areas on the topologies where augmenting paths are
long, 32 failing ties on years around the window length, and the planning model's 8 ELU slots in week 53.  tests/test_hl1_chrono_edges.py
and its _host companion run the sweep, storage and event kernels on the same seq shapes (chrono_shapes), with the storages, sweep levels,
withheld units and coverage conditions defined beside them.  tests/test_hl1_track_edges.py and its _host companion run the weather,
stress, multi-state and area-weather kernels there too (track_shapes, ms_shapes), with the weather libraries, stress multipliers, outage
classes, three-state fleets and the largest area configuration defined below.  Every value is computed here; nothing is read from disk."""
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


# ---- the weather, stress, multi-state and area-weather kernels (tests/test_hl1_track_edges.py and its _host companion) -----------------
EDGE_UNITS = (0, 31, 32, 63, 64, 127)                           # first and last unit of a mask word, of a lane slot, of the largest fleet
MS_NHOURS_EDGES = (1, 24, 63, 64, 65, 255, 256, 257, 511, 512, 513)      # NHOURS_EDGES and the edges of the multi-state kernel's 256-step window
SPIKE = 2.0 ** 60                                               # a multiplier that uses up every draw at once; 2^60 + E == 2^60 for E < 128


def _tool(name):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", "tools", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def edge_weather(load, n_weather, n_res, curves, share=0.06):
    """A weather library for the curve `load` -> (output_mw[n_weather, n_res, H], load curves [n_weather, H] or None).  The outputs are
    multiples of 1/64 MW; resource r gives at most share * (1 + r / 4) / n_res of the mean load, so all of them together stay below
    2 * share of it.  The last resource is identically 0 in weather year 1 (0 if there is one weather year).  With `curves` weather year
    w has the curve load * f_w, f_w spread evenly over 0.94 .. 1.06 (one year: 1.0): the first weather years lose little, the last ones
    much, so two weather years give different records."""
    load = np.asarray(load, dtype=np.float64)
    H = load.size
    rng = np.random.default_rng(7000 + 31 * n_weather + 7 * n_res + H)
    top = share * abs(float(load.mean())) * (1.0 + np.arange(n_res) / 4.0) / max(n_res, 1)
    out = np.floor(rng.uniform(0.0, 1.0, (n_weather, n_res, H)) * top[None, :, None] * 64.0) / 64.0
    if n_res:
        out[min(1, n_weather - 1), n_res - 1, :] = 0.0
    wl = None
    if curves:
        lo, hi = (0.4, 0.6) if H == 1 else (0.6, 1.06)
        f = np.linspace(lo, hi, n_weather) if n_weather > 1 else np.ones(1)
        wl = load[None, :] * f[:, None]
    return out, wl


def spike_hours(H):
    """The hours of edge_stress's spikes: every second hour of a stretch that starts at H // 3 and is about a quarter of the year long
    (three spikes at least, where the year has room for them)."""
    s0 = H // 3
    return list(range(s0, min(H, s0 + max(5, H // 4)), 2))


def edge_stress(n_weather, n_classes, H, spike=SPIKE):
    """fail_mult[n_weather, n_classes, H], n_classes >= 3, dyadic.
      class 0   1/8 .. 3 in steps of 1/8, with zero stretches at the start, in the middle and at the end of weather year 0, and weather
                year 1 (0 if there is one) zero throughout: G[H] == 0 there, so a draw passes that year unchanged
      class 1   as class 0 without the zero stretches, but in the last weather year zero except for SPIKE in every second hour of
                spike_hours(H): a UP unit of the class fails at the start of the first spike; one that becomes UP inside a spike hour
                fails within it; one that becomes UP in the hour between two spikes has t = G[j] + E == G[j] (E < 128 is below half an
                ulp of 2^60), lands on that hour, which has no slope (d == 0), and fails at its end, where the next spike begins.  The
                contract's arithmetic puts each of these failures on a whole hour n exactly (E / 2^60 of an hour is below half an ulp
                of any n >= 1), and a transition at n counts for step n; an hour loop in real arithmetic has it a moment after n, in
                step n + 1.  So hl1_stress_model.literal_stress_chain is held against the model with spike = 2^10, which still fails
                every unit within the hour but absorbs no draw
      class 2   2^-24 in every hour: no unit of it fails before a chain ends
      others    1/4 .. 4 in steps of 1/4, each with a zero stretch of its own
    At H = 1 a row is one hour: class 0 is 1/2, 0, 2, ... over the weather years, class 1 is 1 and SPIKE in the last weather year."""
    assert n_classes >= 3
    rng = np.random.default_rng(8000 + 31 * n_weather + 7 * n_classes + H)
    m = rng.integers(1, 25, (n_weather, n_classes, H)) / 8.0
    m[:, 3:, :] = rng.integers(1, 17, (n_weather, n_classes - 3, H)) / 4.0
    zero_year, spike_year = min(1, n_weather - 1), n_weather - 1
    if H == 1:
        m[:, 0, 0] = [(0.5, 0.0, 2.0)[w % 3] for w in range(n_weather)]
        m[:, 1, 0] = 1.0
        m[spike_year, 1, 0] = spike
    else:
        a, b = max(1, H // 12), max(1, H // 10)
        m[0, 0, :a] = 0.0
        m[0, 0, H // 2 - b // 2:H // 2 - b // 2 + b] = 0.0
        m[0, 0, H - b:] = 0.0
        m[zero_year, 0, :] = 0.0
        m[spike_year, 1, :] = 0.0
        m[spike_year, 1, spike_hours(H)] = spike
        for c in range(3, n_classes):
            s = (c * H) // n_classes
            m[:, c, s:s + a] = 0.0
    m[:, 2, :] = 2.0 ** -24
    return m


def edge_classes(ngen, n_classes=3):
    """unit_class[ngen]: the units of EDGE_UNITS that exist have a class (1, 2, 0, 1, ... in their order, so unit 0 is in the spike
    class), the units next to them that are not EDGE_UNITS themselves have class -1, and the others take -1, 0, 1, ... in turn (unit 2,
    seq_fleet's unit with repairs of minutes, is in class 1 when n_classes is 3).  Every class is used from n_classes + 3 units on."""
    cls = np.array([k % (n_classes + 1) - 1 for k in range(ngen)], dtype=np.int32)
    edge = [k for k in EDGE_UNITS if k < ngen]
    for k in edge:
        for nb in (k - 1, k + 1):
            if 0 <= nb < ngen and nb not in edge:
                cls[nb] = -1
    for i, k in enumerate(edge):
        cls[k] = (i + 1) % n_classes
    return cls


def track_shapes():
    """chrono_shapes() with the weather pick of each: RANDOM (0) on the all-UP shapes, CYCLE (1) on the stationary ones."""
    return [s + (s[6],) for s in chrono_shapes()]


# (pick, n_weather) under which the g*-1 shapes (first_chain = 2^32 - 4, six-year chains) are run so that a weather pick without the
# chain's upper word shows: RANDOM over 3 weather years (the upper word is a Philox counter word), CYCLE over 5 (2^32 * 6 mod 5 = 1; over
# 3 weather years 2^32 * 6 mod 3 = 0: chain 2^32 + j would have chain j's weather years)
UPPER_WORD_PICKS = ((0, 3), (1, 5))


def mixed_weather_groups(W, H, years):
    """The number of 64-step groups (of the 512-step windows) of the chains W[nchains, years] that hold steps of two or more different
    weather years."""
    W = np.asarray(W).reshape(-1, years)
    S = years * H
    n = 0
    for w in W:
        per_step = np.repeat(w, H)
        for g0 in range(0, S, 64):
            n += np.unique(per_step[g0:min(g0 + 64, S)]).size > 1      # 512 is a multiple of 64: the groups of every window start at g0
    return n


def track_coverage(label, cnt, W, H, years):
    """The conditions on a shape's inputs under edge_weather and edge_storages, on the step counters of hl1_variable_model.variable_chain
    and the weather years W: storage_coverage's (short, lost and discharging steps; long, served and charging steps, from which nhours = 1
    is exempt as it is there: its curve has one hour, the all-UP capacity), quiet groups beside serial ones, every weather year of a
    three-year library drawn, and for years shorter than a group some group that holds two weather years."""
    storage_coverage(label, cnt)
    assert 0 < cnt["serial_groups"] < cnt["groups"], (label, cnt)
    assert np.unique(W).size >= 3, (label, np.unique(W))
    if H < 64:
        assert mixed_weather_groups(W, H, years) > 0, label


def stress_coverage(label, cnt, H, ngen):
    """The conditions on a shape's inputs under edge_stress and edge_classes, on hl1_stress_model.stress_chronology's counters: failures
    through the failure time and plain transitions, a draw that no year uses up (`never`), and on every year longer than one hour a draw
    carried across a year, a landing on an hour without slope, and a failure within the hour of the repair.  nhours = 1 is exempt from
    these three: its one-hour rows have no second hour to carry into or land on (a carried draw and an immediate failure do occur and are
    asserted; `flat` cannot).  A fleet of one unit has one class, so it has no failure of a class -1 unit: ngen = 1 is exempt from it."""
    assert cnt["failures"] > 0 and cnt["plain"] > 0 and 0 < cnt["never"] < cnt["failures"], (label, cnt)
    assert cnt["carried"] > 0 and cnt["immediate"] > 0, (label, cnt)
    if H > 1:
        assert cnt["flat"] > 0, (label, cnt)
    if ngen > 1:
        assert cnt["plain_failures"] > 0, (label, cnt)


MS_PATTERNS = ((1.0, 0.3, 0.0), (0.5, 0.0, 1.0), (0.0, 1.0, 1.0))      # first_p of a derated unit beside three_state's, which lies strictly inside


def ms_fleet(ngen, nhours):
    """seq_fleet(ngen, nhours) with three-state units -> (units, two_state_image, load), units as hl1_multistate_model's tuples.
    (hl1_multistate_model.edge_fleet does not do this: it draws capacities and rates of its own, has no derated unit at 0 or 127 and no
    branch probability of 0.)  The units of EDGE_UNITS, every third unit from 2 on and every eighth from 7 on are derated at 0.55 of
    their capacity (rounded to 1/8 MW).  They take in turn, from unit 0 on: MS_PATTERNS[0] (UP always leaves for DOWN, DOWN always for
    DERATED, DERATED for UP three times in ten and for DOWN otherwise: DERATED -> DOWN -> DERATED), three_state's probabilities (all
    strictly inside), MS_PATTERNS[1] (UP leaves for either state, DERATED always for DOWN, DOWN always for UP) and MS_PATTERNS[2] (UP <->
    DERATED only, DOWN out of reach).  Over the four, hl1_ms_kinds' three kinds occur for each of the three states.  The mean times are
    seq_fleet's: mttf in UP, mttr in DOWN, mttr / 2 in DERATED (three_state sets its own from the same two).  The two-state image has
    every unit with first_p (1, 1, 1): relmc_hl1_seq's fleet."""
    MM = _tool("hl1_multistate_model")
    cap, mttf, mttr, load = seq_fleet(ngen, nhours)
    units, i = [], 0
    for k in range(ngen):
        if k in EDGE_UNITS or k % 3 == 2 or k % 8 == 7:
            der = float(np.round(0.55 * cap[k] * 8.0) / 8.0)
            if i % 4 == 1:
                units.append(MM.three_state(cap[k], der, mttf[k], mttr[k]))
            else:
                units.append((float(cap[k]), der, (float(mttf[k]), 0.5 * float(mttr[k]), float(mttr[k])), MS_PATTERNS[(i % 4 + 1) // 2]))
            i += 1
        else:
            units.append(MM.two_state(cap[k], mttf[k], mttr[k]))
    return units, [MM.two_state(cap[k], mttf[k], mttr[k]) for k in range(ngen)], load


def ms_shapes():
    """The multi-state shapes as (label, nhours or ngen arguments of ms_fleet, seed, first_chain, n_chains, years, start): 8 units on
    MS_NHOURS_EDGES under both start rules, and NGEN_EDGES at H = 100 as chrono_shapes() has them."""
    out = []
    for nhours in MS_NHOURS_EDGES:
        for start in (0, 1):
            out.append(("h%d-%d" % (nhours, start), (8, nhours), 13, 40, 8, seq_years(nhours), start))
    for ngen in NGEN_EDGES:
        for start, first in ((0, 0), (1, (1 << 32) - 4)):
            out.append(("g%d-%d" % (ngen, start), (ngen, 100), 3, first, 8, 6, start))
    return out


def ms_coverage(label, nhours, kinds):
    """The conditions on a multi-state shape, on hl1_multistate_model.path_counts: sojourns that cover no step, DERATED -> DOWN -> DERATED
    inside one 64-step group, and sojourns across a group edge, a 256-step window edge and a year boundary.  No year length is exempt:
    every chain runs about 1600 steps, so it has group and window edges whatever the year length, and at nhours = 1 every sojourn of two
    steps crosses a year boundary."""
    assert all(kinds[k] > 0 for k in ("zero", "der_down_der", "group", "window", "year")), (label, nhours, kinds)


def area_var_max_case(nhours):
    """The largest configuration of relmc_hl1_area_var: area_fleet8 (8 areas, 128 units), the 32 ties of topologies8()["complete"], all
    with finite MTTF and MTTR drawn as area_tie_edges draws them, 8 resources (areas 0 and 7 among them, resource 3 at scale 0), 8
    storages (areas 0 and 7 among them) sized to their areas, 3 weather years with load curves per area -> a dict with
    hl1_area_variable_model.shape's keys, and `out` and `wl`."""
    units, cap, mttf, mttr, loads = area_fleet8(nhours)
    ties = topologies8()["complete"][:32]                           # the 28 pairs and four parallel ties with reversed endpoints
    rng = np.random.default_rng(900 + 128)
    kf = rng.uniform(30.0, 200.0, 32)
    kr = rng.uniform(3.0, 30.0, 32)
    kr[2::5] = rng.uniform(0.01, 0.3, kr[2::5].size)
    kf[1::6] = rng.uniform(2.0, 6.0, kf[1::6].size)
    resource_area = [0, 7, 3, 2, 4, 7, 5, 0]
    resource_scale = [1.0, 0.5, 1.25, 0.0, 1.0, 0.75, 1.0, 2.0]
    storage_area = [7, 0, 3, 7, 2, 4, 6, 0]
    mean = loads.mean(axis=1)
    frac = [(0.05, 0.06, 0.2, 0.9, 0.95, 1.0), (0.03, 0.04, 0.1, 1.0, 1.0, 0.0), (0.08, 0.05, 0.3, 0.85, 0.8, 0.5), (0.02, 0.07, 0.15, 1.0, 0.9, 1.0)]
    storages = []
    for i, a in enumerate(storage_area):
        c, d, e, ec, ed, s0 = frac[i % 4]
        storages.append((a, (c * mean[a], d * mean[a], e * mean[a], ec, ed, s0 * (e * mean[a]))))
    n_weather = 3
    rng = np.random.default_rng(9100 + nhours)
    top = np.array([0.06 * (1.0 + r / 4.0) * mean[a] for r, a in enumerate(resource_area)])
    out = np.floor(rng.uniform(0.0, 1.0, (n_weather, 8, nhours)) * top[None, :, None] * 64.0) / 64.0
    out[1, 7, :] = 0.0
    f = 1.0 + 0.05 * np.cos(2.0 * np.pi * (np.arange(n_weather)[:, None] / n_weather + np.arange(8)[None, :] / 8.0))
    wl = loads[None, :, :] * f[:, :, None]
    return dict(units=units, cap=cap, mttf=mttf, mttr=mttr, loads=loads, ties=ties, tie_mttf=kf, tie_mttr=kr, resource_area=resource_area,
                resource_scale=resource_scale, storages=storages, n_weather=n_weather, out=out, wl=wl)


def area_var_tie_case(ngen, nhours):
    """area_tie_edges(ngen, nhours) with 3 resources (areas 3, 0, 3: the odd tail), 2 storages (areas 3 and 1) and 3 weather years with
    load curves per area -> a dict as area_var_max_case's."""
    units, cap, mttf, mttr, loads, ties, kf, kr = area_tie_edges(ngen, nhours)
    resource_area = [3, 0, 3]
    mean = loads.mean(axis=1)
    rng = np.random.default_rng(9200 + nhours + ngen)
    top = np.array([0.08 * (1.0 + r / 4.0) * mean[a] for r, a in enumerate(resource_area)])
    out = np.floor(rng.uniform(0.0, 1.0, (3, 3, nhours)) * top[None, :, None] * 64.0) / 64.0
    out[1, 2, :] = 0.0
    f = 1.0 + 0.05 * np.cos(2.0 * np.pi * (np.arange(3)[:, None] / 3.0 + np.arange(4)[None, :] / 4.0))
    wl = loads[None, :, :] * f[:, :, None]
    storages = [(3, (0.05 * mean[3], 0.06 * mean[3], 0.2 * mean[3], 0.9, 0.95, 0.2 * mean[3])),
                (1, (0.1 * mean[1], 0.1 * mean[1], 0.3 * mean[1], 1.0, 0.8, 0.0))]
    return dict(units=units, cap=cap, mttf=mttf, mttr=mttr, loads=loads, ties=ties, tie_mttf=kf, tie_mttr=kr, resource_area=resource_area,
                resource_scale=[1.0, 0.5, 1.25], storages=storages, n_weather=3, out=out, wl=wl)


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
