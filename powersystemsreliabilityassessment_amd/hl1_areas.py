"""HL1 multi-area generating adequacy with tie-line transfers — GeneratingAdequacy/AdequacyAssessmentII.jl on the GPU.

Mirror of the reference's module AdequacyAssessmentFast:
  TieLine / Area / System (.topology_matrix)        (:28-59)   1-based areas, as the reference
  ISOLATED / INTERCONNECTED                          (:61)
  solve_curtailment_fast(sys, margins, policy, flow) (:73-179)  host port (numpy), no GPU needed; flow="max_flow" is the full
                                                                solver the reference's comment at :136-146 leaves out
  run_fast_sequential_simulation(sys, policy, n_years)(:185-250) the chronological Monte Carlo on the GPU (relmc_hl1_area_load /
                                                                relmc_hl1_area), with per-area and system LOLF / LOLD
  comparison_report(res_iso, res_int)                (:280-291)  the demo's final table (text)
`demo_system()` is the system of `run_demo` (:256-277); `rts96_system()` the three-area IEEE RTS-96 as three RTS-24 fleets joined by
the summed tie capacities of `case96.TIES`.  The units are `hl1.Generator`s; the chronology and its draws are those of
`hl1.run_sequential_mc` (include/relmc.h), so both policies under one seed see the same fleet history.

An extension the reference does not have: a `TieLine` with a finite `mttf` / `mttr` fails and repairs like a unit
(relmc_hl1_area_tie_outages); its draws are apart from the units', so runs with and without tie outages under one seed see the same
fleet too.  `rts96_tie_lines()` / `rts96_system(tie_outages=True)` carry the outage data of `case96.TIES`; `tie_outage_report` is the
table of what tie unreliability costs.
"""
from __future__ import annotations

import ctypes as C
import enum
import math
import time
from dataclasses import dataclass, field
from typing import NamedTuple

import numpy as np

from . import _abi, case96, hl1


@dataclass
class TieLine:                        # :28-32 (1-based areas)
    from_area: int
    to_area: int
    capacity: float
    mttf: float = math.inf            # hours, as hl1.Generator; inf: the tie never fails (the reference's tie)
    mttr: float = math.inf


@dataclass
class Area:                           # :34-39
    id: int
    name: str
    generators: list
    hourly_load: np.ndarray


class SupportPolicy(enum.IntEnum):    # :61 (values = RELMC_HL1_AREA_*)
    ISOLATED = _abi.HL1_AREA_ISOLATED
    INTERCONNECTED = _abi.HL1_AREA_INTERCONNECTED


ISOLATED, INTERCONNECTED = SupportPolicy.ISOLATED, SupportPolicy.INTERCONNECTED
_FLOW = {"reference": _abi.HL1_AREA_FLOW_REFERENCE, "max_flow": _abi.HL1_AREA_FLOW_MAX_FLOW}
_EPS = 1e-4                           # the reference's surplus / deficit / residual threshold (:107-108, :129)
_MAX_AUG = 4096                       # augmentations per step at most (include/relmc.h; a guard)


class System:                         # :41-59
    """Areas and tie lines; topology_matrix[i, j] = summed capacity of the ties between areas i + 1 and j + 1 (both directions)."""

    def __init__(self, areas, tie_lines):
        self.areas = list(areas)
        self.tie_lines = list(tie_lines)
        n = len(self.areas)
        mat = np.zeros((n, n))
        for line in self.tie_lines:
            i, j = int(line.from_area) - 1, int(line.to_area) - 1
            if not (0 <= i < n and 0 <= j < n) or i == j:
                raise ValueError(f"System: tie line {line} must join two different areas among 1..{n}")
            mat[i, j] += line.capacity
            mat[j, i] += line.capacity
        self.topology_matrix = mat


class AreaResult(NamedTuple):         # the reference's (area = ..., lole = ..., eue = ...) of :243-247
    area: str
    lole: float
    eue: float


@dataclass
class MultiAreaResult:
    """run_fast_sequential_simulation's result: `results` is the reference's list of (area, lole, eue); per-area LOLF (events per year)
    and LOLD (hours per event); the system row (a loss hour in any area); per-year indices year_indices[year, row, (loss hours, EUE,
    loss events)], rows = areas then the system, years in chain-major order."""
    policy: SupportPolicy
    flow: str
    results: list
    lolf: np.ndarray
    lold: np.ndarray
    system_lole: float
    system_eue: float
    system_lolf: float
    system_lold: float
    computation_time: float
    year_indices: np.ndarray = field(default_factory=lambda: np.zeros((0, 0, 3)))
    tie_unavailability: np.ndarray = field(default_factory=lambda: np.zeros(0))   # per tie, mttr / (mttf + mttr); 0: never fails


def _augment(m, R, flow: str):
    """The INTERCONNECTED loop of :105-167 (flow "reference") or the max-flow variant, in place on margins m and residuals R (0-based)."""
    n = len(m)

    def bfs(s, t):                    # t >= 0: path to t; t < 0: to the first popped area in deficit
        parent, marked, queue, head = [0] * n, [False] * n, [s], 0
        marked[s] = True
        while head < len(queue):
            u = queue[head]
            head += 1
            if (u == t) if t >= 0 else (m[u] < -_EPS):
                return u, parent
            for v in range(n):
                if R[u][v] > _EPS and not marked[v]:
                    parent[v] = u
                    marked[v] = True
                    queue.append(v)
        return -1, parent

    for _ in range(_MAX_AUG):
        if flow == "reference":
            s = next((i for i in range(n) if m[i] > _EPS), -1)
            t = next((i for i in range(n) if m[i] < -_EPS), -1)
            if s < 0 or t < 0:
                return
            found, parent = bfs(s, t)
            if found < 0:
                return                # the reference's break: no other pair is tried
        else:
            t = -1
            for s in range(n):
                if m[s] > _EPS:
                    t, parent = bfs(s, -1)
                    if t >= 0:
                        break
            if t < 0:
                return
        f = min(m[s], -m[t])
        v = t
        while v != s:
            f = min(f, R[parent[v]][v])
            v = parent[v]
        m[s] -= f
        m[t] += f
        v = t
        while v != s:
            p = parent[v]
            R[p][v] -= f
            R[v][p] += f
            v = p


def _topology_up(sys: System, ties_up) -> list:
    """The per-step T of include/relmc.h: from 0.0, the capacities of the ties that are UP in ascending tie order."""
    up = np.asarray(ties_up, dtype=bool).ravel()
    if up.size != len(sys.tie_lines):
        raise ValueError(f"solve_curtailment_fast: {up.size} tie states for {len(sys.tie_lines)} tie lines")
    n = len(sys.areas)
    T = [[0.0] * n for _ in range(n)]
    for line, u in zip(sys.tie_lines, up):
        if u:
            i, j = int(line.from_area) - 1, int(line.to_area) - 1
            T[i][j] += line.capacity
            T[j][i] += line.capacity
    return T


def solve_curtailment_fast(sys: System, margins, policy, flow: str = "reference", ties_up=None) -> np.ndarray:
    """Curtailment per area for one hour's margins (capacity - load per area, :73-179).  ISOLATED: the negative margins.
    INTERCONNECTED, flow="reference": the reference's augmenting-path loop, which stops at the first surplus area that cannot reach the
    first deficit area.  flow="max_flow": every surplus area is tried, so the total curtailment is the least the ties allow.
    ties_up: optional boolean per tie line, the ties in service this hour (default: all of them)."""
    if flow not in _FLOW:
        raise ValueError(f"solve_curtailment_fast: flow must be one of {sorted(_FLOW)}, not {flow!r}")
    m = [float(x) for x in np.asarray(margins, dtype=np.float64).ravel()]
    if len(m) != len(sys.areas):
        raise ValueError(f"solve_curtailment_fast: {len(m)} margins for {len(sys.areas)} areas")
    T = sys.topology_matrix.tolist() if ties_up is None else _topology_up(sys, ties_up)
    if all(x >= 0 for x in m):
        return np.zeros(len(m))
    if SupportPolicy(policy) == INTERCONNECTED:
        _augment(m, T, flow)
    return np.array([-x if x < 0 else 0.0 for x in m])


_START = {"all_up": _abi.HL1_START_ALL_UP, "stationary": _abi.HL1_START_STATIONARY}


def _flatten(sys: System):
    """Validated device arrays: units area-major, loads [n_areas][nhours], 0-based ties."""
    n = len(sys.areas)
    if not 1 <= n <= _abi.AREA_MAX:
        raise ValueError(f"run_fast_sequential_simulation: {n} areas; 1..{_abi.AREA_MAX} are supported")
    units = np.array([len(a.generators) for a in sys.areas], dtype=np.int32)
    if units.min() < 1 or units.sum() > 128:
        raise ValueError("run_fast_sequential_simulation: every area needs a unit, and 128 units at most in total")
    gens = [g for a in sys.areas for g in a.generators]
    cap, mttf, mttr = (np.ascontiguousarray([getattr(g, f) for g in gens], dtype=np.float64) for f in ("capacity", "mttf", "mttr"))
    if not (np.all(np.isfinite(mttf)) and np.all(mttf > 0) and np.all(np.isfinite(mttr)) and np.all(mttr > 0)):
        raise ValueError("run_fast_sequential_simulation: MTTF and MTTR must be finite and positive")
    H = {np.asarray(a.hourly_load).size for a in sys.areas}
    if len(H) != 1 or H == {0}:
        raise ValueError("run_fast_sequential_simulation: every area needs the same non-empty number of hours")
    load = np.ascontiguousarray(np.stack([np.asarray(a.hourly_load, dtype=np.float64) for a in sys.areas]))
    tf = np.ascontiguousarray([int(t.from_area) - 1 for t in sys.tie_lines], dtype=np.int32)
    tt = np.ascontiguousarray([int(t.to_area) - 1 for t in sys.tie_lines], dtype=np.int32)
    tc = np.ascontiguousarray([t.capacity for t in sys.tie_lines], dtype=np.float64)
    if tf.size and (min(tf.min(), tt.min()) < 0 or max(tf.max(), tt.max()) >= n or np.any(tf == tt)):
        raise ValueError("run_fast_sequential_simulation: a tie line must join two different areas among 1..n")
    if not (np.all(np.isfinite(tc)) and np.all(tc >= 0)):
        raise ValueError("run_fast_sequential_simulation: tie capacities must be finite and >= 0")
    return units, cap, mttf, mttr, load, tf, tt, tc


def _tie_outages(sys: System):
    """Validated (mttf, mttr) of the tie lines, or (None, None) when no tie fails (every mttf = inf)."""
    kf = np.ascontiguousarray([t.mttf for t in sys.tie_lines], dtype=np.float64)
    kr = np.ascontiguousarray([t.mttr for t in sys.tie_lines], dtype=np.float64)
    fails = np.isfinite(kf)
    if np.any(np.isnan(kf)) or np.any(kf <= 0) or not (np.all(np.isfinite(kr[fails])) and np.all(kr[fails] > 0)):
        raise ValueError("run_fast_sequential_simulation: a tie's MTTF must be > 0 (inf: it never fails), a failing tie's MTTR finite and > 0")
    if not fails.any():
        return None, None
    if kf.size > _abi.HL1_TIE_MAX:
        raise ValueError(f"run_fast_sequential_simulation: {kf.size} tie lines with outage data; {_abi.HL1_TIE_MAX} at most")
    return kf, np.where(fails, kr, 1.0)                  # a tie that never fails: its MTTR is not read


def _model_load(eng, units, cap, mttf, mttr, load, tf, tt, tc, kf, kr) -> None:
    """relmc_hl1_area_load (and the tie outage data) unless the engine already holds this very model: areas, ties, outage data and loads
    stay on the device between calls on the same system."""
    L = eng.L
    dp, ip = _abi.c_double_p, _abi.c_int32_p
    key = tuple(a.tobytes() for a in (units, cap, mttf, mttr, load, tf, tt, tc)) + ((kf.tobytes(), kr.tobytes()) if kf is not None else ())
    if getattr(eng, "_hl1_area_loaded", None) != key:
        eng._check(L.relmc_hl1_area_load(eng._h, units.size, units.ctypes.data_as(ip), cap.ctypes.data_as(dp), mttf.ctypes.data_as(dp),
                                         mttr.ctypes.data_as(dp), load.shape[1], load.ctypes.data_as(dp), tf.size,
                                         tf.ctypes.data_as(ip), tt.ctypes.data_as(ip), tc.ctypes.data_as(dp)), "relmc_hl1_area_load")
        if kf is not None:                                  # the load has cleared any earlier outage data
            eng._check(L.relmc_hl1_area_tie_outages(eng._h, kf.size, kf.ctypes.data_as(dp), kr.ctypes.data_as(dp)), "relmc_hl1_area_tie_outages")
        eng._hl1_area_loaded = key


def run_fast_sequential_simulation(sys: System, policy, n_years: int, *, seed: int = 1, chains: int = 1, start: str = "all_up",
                                   flow: str = "reference", engine=None) -> MultiAreaResult:
    """AdequacyAssessmentII.jl:185-250 on the GPU: `chains` chronological chains of n_years // chains years each; every step takes each
    area's margin and, under INTERCONNECTED, the tie-limited transfer solve (`flow` as in solve_curtailment_fast).  The defaults are the
    reference's shape (one chain, every unit UP at the start).  Runs of both policies under one seed see the same fleet history, so
    their difference is the interconnection benefit without sampling noise between them."""
    from . import api
    n_years, chains = int(n_years), int(chains)
    if n_years < 1 or chains < 1 or n_years % chains:
        raise ValueError(f"run_fast_sequential_simulation: n_years ({n_years}) must be a positive multiple of chains ({chains})")
    if start not in _START:
        raise ValueError(f"run_fast_sequential_simulation: start must be one of {sorted(_START)}, not {start!r}")
    if flow not in _FLOW:
        raise ValueError(f"run_fast_sequential_simulation: flow must be one of {sorted(_FLOW)}, not {flow!r}")
    if policy not in (ISOLATED, INTERCONNECTED):
        raise ValueError(f"run_fast_sequential_simulation: policy must be ISOLATED or INTERCONNECTED, not {policy!r}")
    policy = SupportPolicy(policy)
    units, cap, mttf, mttr, load, tf, tt, tc = _flatten(sys)
    kf, kr = _tie_outages(sys)
    eng = engine or api.default_engine()
    L = eng.L
    t0 = time.time()
    n = units.size
    _model_load(eng, units, cap, mttf, mttr, load, tf, tt, tc, kf, kr)
    acc = (_abi.Hl1SeqAcc * (n + 1))()
    yr = np.zeros((n_years, n + 1, 3))
    eng._check(L.relmc_hl1_area(eng._h, int(seed), 0, chains, n_years // chains, _START[start], int(policy), _FLOW[flow], acc,
                                yr.ctypes.data_as(C.POINTER(_abi.Hl1SeqYear))), "relmc_hl1_area")
    lole = np.array([a.sum_lole for a in acc]) / n_years
    eue = np.array([a.sum_eue for a in acc]) / n_years
    lolf = np.array([a.sum_lolf for a in acc]) / n_years
    with np.errstate(invalid="ignore", divide="ignore"):
        lold = np.where(lolf > 0, lole / np.where(lolf > 0, lolf, 1.0), np.nan)
    return MultiAreaResult(policy, flow, [AreaResult(a.name, float(lole[i]), float(eue[i])) for i, a in enumerate(sys.areas)],
                           lolf[:n].copy(), lold[:n].copy(), float(lole[n]), float(eue[n]), float(lolf[n]), float(lold[n]),
                           time.time() - t0, yr,
                           np.zeros(tf.size) if kf is None else np.where(np.isfinite(kf), kr / (np.where(np.isfinite(kf), kf, 1.0) + kr), 0.0))


def comparison_report(res_iso: MultiAreaResult, res_int: MultiAreaResult) -> str:
    """The final table of run_demo (:280-291)."""
    rule = "-" * 60
    lines = ["", "=== FINAL COMPARISON (FAST METHOD) ===", "Policy          | Area       | LOLE (h/yr) | EUE (MWh/yr)", rule]
    lines += ["ISOLATED        | %-10s | %10.2f  | %10.2f" % (r.area, r.lole, r.eue) for r in res_iso.results]
    lines.append(rule)
    lines += ["INTERCONNECTED  | %-10s | %10.2f  | %10.2f" % (r.area, r.lole, r.eue) for r in res_int.results]
    return "\n".join(lines) + "\n"


def tie_outage_report(res_perfect: MultiAreaResult, res_outage: MultiAreaResult) -> str:
    """INTERCONNECTED with ties that never fail against INTERCONNECTED with failing ties, per area and for the system.  Under one seed both
    runs see the same fleet history, so the differences are the cost of tie unreliability without fleet sampling noise between the runs."""
    rule = "-" * 76
    lines = ["", "=== TIE OUTAGES (INTERCONNECTED) ===", "Ties            | Area       | LOLE (h/yr) | EUE (MWh/yr) | LOLF (occ/yr)", rule]
    for label, res in (("PERFECT", res_perfect), ("FAILING", res_outage)):
        lines += ["%-15s | %-10s | %10.2f  | %11.2f  | %10.4f" % (label, r.area, r.lole, r.eue, f) for r, f in zip(res.results, res.lolf)]
        lines.append("%-15s | %-10s | %10.2f  | %11.2f  | %10.4f" % (label, "SYSTEM", res.system_lole, res.system_eue, res.system_lolf))
        lines.append(rule)
    lines += ["DIFFERENCE      | %-10s | %10.2f  | %11.2f  | %10.4f" % (a.area, b.lole - a.lole, b.eue - a.eue, fb - fa)
              for a, b, fa, fb in zip(res_perfect.results, res_outage.results, res_perfect.lolf, res_outage.lolf)]
    lines.append("DIFFERENCE      | %-10s | %10.2f  | %11.2f  | %10.4f" % ("SYSTEM", res_outage.system_lole - res_perfect.system_lole,
                                                                      res_outage.system_eue - res_perfect.system_eue,
                                                                      res_outage.system_lolf - res_perfect.system_lolf))
    return "\n".join(lines) + "\n"


# ---- sweep of the multi-area model on one chronology: load, tie and fleet levels (an extension beyond the reference) ---------------------
@dataclass(frozen=True)
class AreaSweepLevel:
    """One level of run_area_sweep: area a sees the load load_scale[a] * load_a + load_shift[a] (a scalar applies to every area), every
    scaled tie has tie_scale times its capacity, and with withheld=True the fleet is the one without the sweep's withheld units."""
    load_scale: object = 1.0
    load_shift: object = 0.0
    tie_scale: float = 1.0
    withheld: bool = False


@dataclass
class AreaSweepResult:
    """run_area_sweep's result: lole / eue / lolf [n_levels, n_areas + 1] (row n_areas = the system: a loss hour in any area), their
    standard errors over the simulated years (NaN with a single year), and year_indices[level, year, row, (loss hours, EUE, loss
    events)] with the years in chain-major order."""
    levels: list
    withheld_units: tuple
    scaled_ties: tuple
    flow: str
    years: int
    areas: list
    lole: np.ndarray
    eue: np.ndarray
    lolf: np.ndarray
    lole_se: np.ndarray
    eue_se: np.ndarray
    lolf_se: np.ndarray
    year_indices: np.ndarray
    computation_time: float


def _area_levels(who: str, sys: System, levels, withheld_units, scaled_ties) -> tuple:
    """The checks of a sweep's levels and masks that need no device -> ([(scale[n], shift[n], tie_scale, withheld)], withheld units,
    scaled tie flags or None)."""
    n, n_units, n_ties = len(sys.areas), sum(len(a.generators) for a in sys.areas), len(sys.tie_lines)
    lv = [x if isinstance(x, AreaSweepLevel) else AreaSweepLevel(*x) for x in levels]
    if not 1 <= len(lv) <= _abi.HL1_AREA_SWEEP_MAX_LEVELS:
        raise ValueError(f"{who}: between 1 and {_abi.HL1_AREA_SWEEP_MAX_LEVELS} levels, not {len(lv)}")
    out = []
    for j, x in enumerate(lv):
        row = []
        for name in ("load_scale", "load_shift"):
            v = np.asarray(getattr(x, name), dtype=np.float64)
            if v.ndim > 1 or (v.ndim == 1 and v.size != n):
                raise ValueError(f"{who}: {name} of level {j} must be a scalar or one value per area ({n})")
            v = np.ascontiguousarray(np.broadcast_to(v, (n,)))
            if not np.all(np.isfinite(v)):
                raise ValueError(f"{who}: {name} of level {j} not finite")
            row.append(v)
        ts = float(x.tie_scale)
        if not (np.isfinite(ts) and ts >= 0.0):
            raise ValueError(f"{who}: tie_scale of level {j} must be finite and >= 0, not {x.tie_scale!r}")
        out.append((row[0], row[1], ts, bool(x.withheld)))
    wh = [int(k) for k in withheld_units]
    if len(set(wh)) != len(wh) or any(not 0 <= k < n_units for k in wh):
        raise ValueError(f"{who}: withheld_units must be distinct global unit indices in [0, {n_units}), not {list(withheld_units)}")
    if not wh and any(x[3] for x in out):
        raise ValueError(f"{who}: a level with withheld=True needs withheld_units")
    mask = None
    if scaled_ties is not None:
        st = [int(t) for t in scaled_ties]
        if len(set(st)) != len(st) or any(not 0 <= t < n_ties for t in st):
            raise ValueError(f"{who}: scaled_ties must be distinct tie indices in [0, {n_ties}), not {list(scaled_ties)}")
        mask = np.zeros(n_ties, dtype=np.uint8)
        mask[st] = 1
    return lv, out, tuple(sorted(wh)), mask


def level_system(sys: System, level, *, withheld_units=(), scaled_ties=None) -> System:
    """The system one level of run_area_sweep is equivalent to, bit for bit: the level's load curves (scale * load + shift, each rounded),
    the scaled tie capacities, and with withheld=True the withheld units at capacity 0.0 (they keep their places and their draws)."""
    _, (lv,), wh, mask = _area_levels("level_system", sys, [level], withheld_units, scaled_ties)
    scale, shift, ts, withheld = lv
    areas, k = [], 0
    for i, a in enumerate(sys.areas):
        gens = [hl1.Generator(g.id, 0.0 if withheld and k + q in wh else g.capacity, g.mttf, g.mttr) for q, g in enumerate(a.generators)]
        k += len(gens)
        areas.append(Area(a.id, a.name, gens, scale[i] * np.asarray(a.hourly_load, dtype=np.float64) + shift[i]))
    ties = [TieLine(t.from_area, t.to_area, ts * t.capacity if mask is None or mask[q] else t.capacity, t.mttf, t.mttr)
            for q, t in enumerate(sys.tie_lines)]
    return System(areas, ties)


def run_area_sweep(sys: System, n_years: int, levels, *, withheld_units=(), scaled_ties=None, seed: int = 1, chains: int = 1,
                   start: str = "all_up", flow: str = "max_flow", engine=None) -> AreaSweepResult:
    """run_fast_sequential_simulation(sys, INTERCONNECTED, ...)'s chronology (same chains under the same seed, tie outages included) against
    up to 8 levels of load, tie capacity and fleet in one walk of the chains (relmc_hl1_area_sweep).  `withheld_units` are 0-based global
    unit indices (area-major); `scaled_ties` the 0-based ties a level's tie_scale applies to (default: every tie).  Level j is bitwise
    run_fast_sequential_simulation on level_system(sys, levels[j], ...); AreaSweepLevel() is the system itself and tie_scale=0 (every tie
    scaled) the ISOLATED policy.  Every level sees the same unit and tie history, so two levels may be differenced year by year.
    Only the system row under flow="max_flow" is monotone in a load shift and in the tie scale, and only up to the solve's 1e-4
    thresholds; an area's own row, and any row under flow="reference", need not be."""
    from . import api
    who = "run_area_sweep"
    n_years, chains = hl1._seq_shape(who, n_years, chains, start)
    if flow not in _FLOW:
        raise ValueError(f"{who}: flow must be one of {sorted(_FLOW)}, not {flow!r}")
    lv, rows, wh, mask = _area_levels(who, sys, levels, withheld_units, scaled_ties)
    units, cap, mttf, mttr, load, tf, tt, tc = _flatten(sys)
    kf, kr = _tie_outages(sys)
    eng = engine or api.default_engine()
    t0 = time.time()
    n, nl = units.size, len(rows)
    _model_load(eng, units, cap, mttf, mttr, load, tf, tt, tc, kf, kr)
    arr = (_abi.Hl1AreaLevel * nl)()
    for j, (scale, shift, ts, withheld) in enumerate(rows):
        arr[j].load_scale[:n] = scale.tolist()
        arr[j].load_shift[:n] = shift.tolist()
        arr[j].tie_scale, arr[j].fleet, arr[j].reserved = ts, 1 if withheld else 0, 0
    wmask = None
    if wh:
        wmask = (C.c_uint32 * 4)()
        for k in wh:
            wmask[k >> 5] |= 1 << (k & 31)
    acc = (_abi.Hl1SeqAcc * (nl * (n + 1)))()
    yr = np.zeros((nl, n_years, n + 1, 3))
    eng._check(eng.L.relmc_hl1_area_sweep(eng._h, int(seed), 0, chains, n_years // chains, _START[start], _FLOW[flow], nl, arr, wmask,
                                          None if mask is None else mask.ctypes.data_as(_abi.c_uint8_p), acc,
                                          yr.ctypes.data_as(C.POINTER(_abi.Hl1SeqYear))), "relmc_hl1_area_sweep")
    mean = lambda f: np.array([getattr(a, f) for a in acc]).reshape(nl, n + 1) / n_years
    se = [hl1._se(np.moveaxis(yr[..., q], 1, -1)) for q in range(3)]
    return AreaSweepResult(lv, wh, tuple(range(tf.size)) if mask is None else tuple(int(t) for t in np.nonzero(mask)[0]), flow, n_years,
                           [a.name for a in sys.areas], mean("sum_lole"), mean("sum_eue"), mean("sum_lolf"), se[0], se[1], se[2], yr,
                           time.time() - t0)


def area_sweep_report(result: AreaSweepResult) -> str:
    """The levels of a sweep, per area and for the system, as a text table in tie_outage_report's style."""
    rule = "-" * 96
    lines = ["", "=== MULTI-AREA SWEEP (INTERCONNECTED, %s) ===" % result.flow,
             "Level | Ties   | Fleet | Area       | LOLE (h/yr) +- SE      | EUE (MWh/yr) +- SE        | LOLF (occ/yr)", rule]
    names = list(result.areas) + ["SYSTEM"]
    for j, lv in enumerate(result.levels):
        for r, name in enumerate(names):
            lines.append("%-5d | x%-5.3g | %-5s | %-10s | %10.2f +- %-8.2f | %12.2f +- %-9.2f | %10.4f" % (
                j, lv.tie_scale, "w/o" if lv.withheld else "all", name, result.lole[j, r], result.lole_se[j, r], result.eue[j, r],
                result.eue_se[j, r], result.lolf[j, r]))
        sc, sh = np.atleast_1d(np.asarray(lv.load_scale, dtype=float)), np.atleast_1d(np.asarray(lv.load_shift, dtype=float))
        lines.append("      load scale %s, shift %s MW" % (", ".join("%g" % v for v in sc), ", ".join("%g" % v for v in sh)))
        lines.append(rule)
    if result.withheld_units:
        lines.append("w/o: the fleet without units %s" % list(result.withheld_units))
    return "\n".join(lines) + "\n"


_AREA_METRIC = {"lole": 0, "eue": 1}


def _first_crossing(who: str, m, target: float) -> int:
    """Index i of the FIRST adjacent pair (i, i + 1) with target between m[i] and m[i + 1] (either order).  The curve need not be sorted:
    only the system row under max_flow is monotone, so no search on the sorted values is made.  ValueError when no pair brackets."""
    m = np.asarray(m, dtype=np.float64)
    for i in range(m.size - 1):
        if min(m[i], m[i + 1]) <= target <= max(m[i], m[i + 1]):
            return i
    raise ValueError(f"{who}: no adjacent pair of levels brackets the target {target:g} (the metric takes {', '.join('%g' % v for v in m)} "
                     "over the bracket)")


def _interpolate_pair(x, m, i: int, target: float) -> tuple:
    """hl1._interpolate inside the pair (i, i + 1), for a pair that rises or falls: (value, weight of level i + 1, slope)."""
    if m[i + 1] >= m[i]:
        return hl1._interpolate(x, m, i, target)
    value, t, slope = hl1._interpolate(np.array([x[i + 1], x[i]]), np.array([m[i + 1], m[i]]), 0, target)
    return value, 1.0 - t, slope


def _area_search(who: str, sys: System, area, n_years, metric, row, bracket, rounds, target, target_level, kw) -> hl1.CarryingCapabilityResult:
    """The search the three functions below share: rounds of load shifts in `area`, equally spaced over the bracket, swept under one seed
    (8 levels, or 7 and the target level); each round keeps the first adjacent pair that brackets the target; the last pair is
    interpolated linearly.  The standard error is the delta method's: that of the metric (of the per-year paired difference to the target
    level, when there is one) over the local slope."""
    n = len(sys.areas)
    if metric not in _AREA_METRIC:
        raise ValueError(f"{who}: metric must be one of {sorted(_AREA_METRIC)}, not {metric!r} (the sampled LOLF is not monotone)")
    if row not in ("area", "system"):
        raise ValueError(f"{who}: row must be 'area' or 'system', not {row!r}")
    if not (isinstance(area, (int, np.integer)) and 1 <= int(area) <= n):
        raise ValueError(f"{who}: area must be one of 1..{n} (1-based, as TieLine), not {area!r}")
    lo, hi, rounds = hl1._search_args(who, "lole", "shift", bracket, rounds)
    hl1._seq_shape(who, n_years, kw.get("chains", 1), kw.get("start", "all_up"))
    a, q, t0 = int(area) - 1, _AREA_METRIC[metric], time.time()
    r = a if row == "area" else n
    nx = _abi.HL1_AREA_SWEEP_MAX_LEVELS - (0 if target_level is None else 1)
    shifted = lambda v: AreaSweepLevel(load_shift=[float(v) if b == a else 0.0 for b in range(n)])
    target_year = []
    for _ in range(rounds):
        x = np.linspace(lo, hi, nx)
        sw = run_area_sweep(sys, n_years, [shifted(v) for v in x] + ([] if target_level is None else [target_level]), **kw)
        m = (sw.lole, sw.eue)[q][:nx, r]
        if target_level is not None:
            target = float((sw.lole, sw.eue)[q][nx, r])
            target_year.append(sw.year_indices[nx, :, r, q].copy())
        i = _first_crossing(who, m, target)
        lo, hi = float(x[i]), float(x[i + 1])
    value, t, slope = _interpolate_pair(x, m, i, target)
    yr = sw.year_indices[:, :, r, q]
    if target_level is None:
        se_m = float((sw.lole_se, sw.eue_se)[q][i + 1 if t > 0.5 else i, r])
    else:
        se_m = float(hl1._se((1.0 - t) * yr[i] + t * yr[i + 1] - yr[nx]))
    return hl1.CarryingCapabilityResult("Multi-area sequential MC sweep", metric, "shift", value, se_m / abs(slope) if slope != 0 else float("inf"),
                                        (lo, hi), (float(m[i]), float(m[i + 1])), float(target), int(n_years), rounds, time.time() - t0, target_year)


def area_load_carrying_capability(sys: System, area: int, target: float, n_years: int, *, metric: str = "lole", row: str = "area", bracket,
                                  rounds: int = 3, withheld_units=(), seed: int = 1, chains: int = 1, start: str = "all_up",
                                  flow: str = "max_flow", engine=None) -> hl1.CarryingCapabilityResult:
    """The load shift (MW, every hour) in area `area` (1-based, as TieLine) at which the sampled metric -- LOLE in h/yr or EUE in MWh/yr, of
    that area (row="area") or of the system (row="system") -- meets `target`.  Each round sweeps 8 equally spaced shifts over the bracket
    under the same seed and narrows the bracket to the FIRST adjacent pair of levels that brackets the target; the last pair is
    interpolated linearly.  Only the system row under flow="max_flow" is monotone in the load (up to the solve's 1e-4 thresholds); an
    area's own row need not be, so the search never assumes a sorted curve, and raises ValueError when no pair brackets the target."""
    return _area_search("area_load_carrying_capability", sys, area, n_years, metric, row, bracket, rounds, float(target), None,
                        dict(withheld_units=withheld_units, seed=seed, chains=chains, start=start, flow=flow, engine=engine))


def interconnection_benefit(sys: System, area: int, n_years: int, *, metric: str = "lole", row: str = "area", bracket=None, rounds: int = 3,
                            seed: int = 1, chains: int = 1, start: str = "all_up", flow: str = "max_flow",
                            engine=None) -> hl1.CarryingCapabilityResult:
    """How much more load area `area` (1-based) carries because it is interconnected: the load shift in that area after which the
    interconnected row is as risky as the isolated one at the unshifted load.  Each round sweeps 7 shifted levels and one tie_scale = 0
    level, the paired target (bitwise ISOLATED, the same in every round); both see the same draws, so the standard error comes from the
    per-year paired differences over the slope.  The default bracket is (0, 1.25 x the capacity of the ties at the area): the benefit
    cannot exceed that capacity, the quarter beyond it is room for the sampling noise.  The first adjacent
    pair that brackets the target is taken (the curve of an area's own row need not be monotone); ValueError when none does."""
    who = "interconnection_benefit"
    if bracket is None and isinstance(area, (int, np.integer)):
        bracket = (0.0, 1.25 * sum(t.capacity for t in sys.tie_lines if int(area) in (t.from_area, t.to_area)))
    return _area_search(who, sys, area, n_years, metric, row, bracket if bracket is not None else (0.0, 0.0), rounds, None,
                        AreaSweepLevel(tie_scale=0.0), dict(seed=seed, chains=chains, start=start, flow=flow, engine=engine))


def unit_elcc(sys: System, units, area: int, n_years: int, *, metric: str = "lole", row: str = "area", bracket=None, rounds: int = 3,
              seed: int = 1, chains: int = 1, start: str = "all_up", flow: str = "max_flow", engine=None) -> hl1.CarryingCapabilityResult:
    """What the units `units` (0-based global indices, area-major) are worth in load of area `area` (1-based) once neighbours can lean on
    them: the load shift in that area after which the whole fleet is as risky as the fleet without the units at the unshifted load.  The
    search of interconnection_benefit with a withheld-fleet level as the paired target.  The default bracket is (0, the units' capacity)."""
    who = "unit_elcc"
    gens = [g for a in sys.areas for g in a.generators]
    wh = [int(k) for k in units]
    if not wh or len(set(wh)) != len(wh) or any(not 0 <= k < len(gens) for k in wh):
        raise ValueError(f"{who}: units must be distinct global unit indices in [0, {len(gens)}), one at least, not {list(units)}")
    if bracket is None:
        bracket = (0.0, sum(gens[k].capacity for k in wh))
    return _area_search(who, sys, area, n_years, metric, row, bracket, rounds, None, AreaSweepLevel(withheld=True),
                        dict(withheld_units=wh, seed=seed, chains=chains, start=start, flow=flow, engine=engine))


# ---- data ---------------------------------------------------------------------------------------------------------------------
def demo_system(hours: int = 8760) -> System:
    """run_demo's system (:259-269): Area_Rich 5 x 400 MW (MTTF 1000 h, MTTR 50 h), Area_Poor 5 x 200 MW (900 h, 60 h), one 200 MW tie;
    loads c + a sin(linspace(0, 2 pi, hours)) (the last bits may differ from Julia's range)."""
    x = np.sin(np.linspace(0.0, 2.0 * np.pi, hours))
    rich = Area(1, "Area_Rich", [hl1.Generator(i, 400.0, 1000.0, 50.0) for i in range(1, 6)], 1000.0 + 500.0 * x)
    poor = Area(2, "Area_Poor", [hl1.Generator(i, 200.0, 900.0, 60.0) for i in range(1, 6)], 800.0 + 400.0 * x)
    return System([rich, poor], [TieLine(1, 2, 200.0)])


def rts96_ties() -> list:
    """case96.TIES summed per area pair (bus number // 100 = area; bus 325 is in area 3): A-B 1175 MW, A-C 500 MW, B-C 500 MW.  The
    323-325 transformer lies inside area C and is dropped."""
    tot = {}
    for fb, tb, *_rest in case96.TIES:
        i, j = sorted((fb // 100, tb // 100))
        if i != j:
            tot[(i, j)] = tot.get((i, j), 0.0) + _rest[1]
    return [TieLine(i, j, c) for (i, j), c in sorted(tot.items())]


def rts96_tie_lines(outages: bool = True) -> list:
    """The five inter-area lines of case96.TIES one by one (107-203, 113-215, 123-217, 325-121, 318-223; the 323-325 transformer lies
    inside area C), capacity = column 4; with `outages`, MTTF = 8760 / lambda and MTTR = the outage duration (columns 5 and 6, the
    conventions of seqmeantime.m:21-36 that seq.py uses)."""
    out = []
    for fb, tb, _x, cap, lam, dur in case96.TIES:
        i, j = sorted((fb // 100, tb // 100))
        if i != j:
            out.append(TieLine(i, j, cap, 8760.0 / lam, dur) if outages else TieLine(i, j, cap))
    return out


def rts96_system(tie_outages: bool = False) -> System:
    """The three-area IEEE RTS-96: three RTS-24 fleets (32 units each) with the RTS-24 load curve each, joined by rts96_ties(), or with
    `tie_outages` by the five failing lines of rts96_tie_lines()."""
    areas = [Area(k + 1, name, hl1.rts24_generators(), hl1.rts24_load().hourly_load) for k, name in enumerate(("A", "B", "C"))]
    return System(areas, rts96_tie_lines() if tie_outages else rts96_ties())
