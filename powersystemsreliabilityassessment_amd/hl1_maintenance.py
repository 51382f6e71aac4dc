"""Planned maintenance on the HL1 sequential chronology — an extension beyond the reference, whose planning scripts know maintenance only
on independently drawn hours (generating_adequancy_comparative.jl; here hl1_planning.py), without frequency, duration or carry-over.

A schedule is a list of MaintenanceWindow(unit, start_hour, hours): unit (0-based index into the fleet) is on maintenance in the hours
start_hour .. start_hour + hours - 1 of every year, taken modulo the year's length.  A unit on maintenance adds nothing to the hour's
capacity; its failure and repair process runs on.  Up to 8 schedules are compared on ONE fleet history (relmc_hl1_maint_load /
relmc_hl1_maint_seq, the contract is written out in include/relmc.h), so two schedules may be differenced year by year.

  MaintenanceWindow(unit, start_hour, hours)
  schedule_from_planning(units)                      the start weeks of hl1_planning.PlanningUnit as windows
  levelised_schedule(generators, load, weeks)        hl1_planning.schedule_maintenance on the chronology's fleet
  run_sequential_maintenance(generators, load, schedules, n_years)   run_sequential_mc's chronology under every schedule, on the GPU
  run_analytical_maintenance(generators, load, schedules)            the exact stationary LOLE / EUE: one COPT per distinct maintenance set
  compare_schedules(result, base)                    paired differences to one schedule, with the standard error of the per-year differences
  maintenance_report(result)                         the table (text)
"""
from __future__ import annotations

import ctypes as C
import time
from dataclasses import dataclass

import numpy as np

from . import _abi, hl1, hl1_planning

MAX_SCHEDULES = _abi.HL1_MAINT_MAX_SCHEDULES


@dataclass(frozen=True)
class MaintenanceWindow:
    """Unit `unit` (0-based) is on maintenance in hours start_hour .. start_hour + hours - 1 of the year (0-based, modulo the year)."""
    unit: int
    start_hour: int
    hours: int


@dataclass
class MaintenanceResult:
    """run_sequential_maintenance's result: index j is schedule j.  The standard errors are over the simulated years (NaN with one year)."""
    schedules: list
    years: int
    lole_hours_yr: np.ndarray
    eue_mwh_yr: np.ndarray
    lolf_occ_yr: np.ndarray
    lole_se: np.ndarray
    eue_se: np.ndarray
    lolf_se: np.ndarray
    year_lole: np.ndarray             # [n_schedules, years], chain-major as run_sequential_mc's
    year_eue: np.ndarray
    year_lolf: np.ndarray
    computation_time: float

    def result(self, j: int) -> hl1.SequentialReliabilityResult:
        """Schedule j as run_sequential_mc would report it (hl1.compare_results takes it)."""
        lole, eue, lolf = float(self.lole_hours_yr[j]), float(self.eue_mwh_yr[j]), float(self.lolf_occ_yr[j])
        k = np.arange(10, self.years + 1, 10)
        history = np.cumsum(self.year_lole[j])[k - 1] / k if k.size else np.zeros(0)
        return hl1.SequentialReliabilityResult("Schedule %d" % j, lole, eue, self.computation_time, history, lolf_occ_yr=lolf,
                                               lold_hours=lole / lolf if lolf > 0 else float("nan"), year_lole=self.year_lole[j].copy(),
                                               year_eue=self.year_eue[j].copy(), year_lolf=self.year_lolf[j].copy())


@dataclass
class AnalyticalMaintenance:
    """run_analytical_maintenance's result: exact stationary LOLE and EUE per schedule, and how many COPTs each took."""
    lole_hours_yr: np.ndarray
    eue_mwh_yr: np.ndarray
    n_copt: np.ndarray
    computation_time: float


@dataclass
class ScheduleComparison:
    """compare_schedules' result: schedule j minus schedule `base`, index j.  *_se is the standard error of the mean per-year difference
    (paired: both schedules saw the same fleet history), *_se_unpaired what two independent runs of the same length would give."""
    base: int
    d_lole: np.ndarray
    d_eue: np.ndarray
    d_lolf: np.ndarray
    d_lole_se: np.ndarray
    d_eue_se: np.ndarray
    d_lolf_se: np.ndarray
    d_lole_se_unpaired: np.ndarray
    d_eue_se_unpaired: np.ndarray
    d_lolf_se_unpaired: np.ndarray


def _schedules(who: str, schedules, n_units: int, n_hours: int) -> list:
    """The checks that need no device; returns a list of lists of MaintenanceWindow."""
    out = [[w if isinstance(w, MaintenanceWindow) else MaintenanceWindow(*w) for w in s] for s in schedules]
    if not 1 <= len(out) <= MAX_SCHEDULES:
        raise ValueError(f"{who}: between 1 and {MAX_SCHEDULES} schedules, not {len(out)}")
    for j, s in enumerate(out):
        for i, w in enumerate(s):
            for name, v in (("unit", w.unit), ("start_hour", w.start_hour), ("hours", w.hours)):
                if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                    raise ValueError(f"{who}: schedule {j}, window {i}: {name} must be an integer, not {v!r}")
            if not 0 <= w.unit < n_units:
                raise ValueError(f"{who}: schedule {j}, window {i}: unit {w.unit} not in [0, {n_units})")
            if not 0 <= w.start_hour < n_hours:
                raise ValueError(f"{who}: schedule {j}, window {i}: start_hour {w.start_hour} not in [0, {n_hours})")
            if not 1 <= w.hours <= n_hours:
                raise ValueError(f"{who}: schedule {j}, window {i}: hours {w.hours} not in [1, {n_hours}]")
    return out


def _curve(who: str, load: hl1.LoadModel, scale, shift) -> np.ndarray:
    scale, shift = float(scale), float(shift)
    if not (np.isfinite(scale) and np.isfinite(shift)):
        raise ValueError(f"{who}: scale / shift not finite")
    return np.float64(scale) * np.asarray(load.hourly_load, dtype=np.float64) + np.float64(shift)


def maintenance_mask(schedule, n_units: int, n_hours: int) -> np.ndarray:
    """on[h, k]: unit k is on maintenance at hour-of-year h under `schedule` ((h - start_hour) mod H < hours for some window of k)."""
    on = np.zeros((n_hours, n_units), dtype=bool)
    h = np.arange(n_hours)
    for w in schedule:
        on[:, w.unit] |= (h - w.start_hour) % n_hours < w.hours
    return on


def schedule_from_planning(units, hours_per_week: int = hl1_planning.HOURS_PER_WEEK) -> list:
    """The schedule that hl1_planning's units carry: unit k with scheduled_outage_start s >= 1 (1-based week) and m maintenance weeks is on
    maintenance in hours (s - 1) * hours_per_week .. (s - 1 + m) * hours_per_week - 1.  Start week 0, or no weeks, means no window."""
    hpw = int(hours_per_week)
    if hpw < 1:
        raise ValueError(f"schedule_from_planning: hours_per_week ({hours_per_week}) must be positive")
    return [MaintenanceWindow(k, (int(u.scheduled_outage_start) - 1) * hpw, int(u.maintenance_weeks) * hpw)
            for k, u in enumerate(units) if int(u.scheduled_outage_start) >= 1 and int(u.maintenance_weeks) >= 1]


def levelised_schedule(generators, load: hl1.LoadModel, weeks, n_weeks: int = hl1_planning.N_WEEKS) -> list:
    """hl1_planning.schedule_maintenance (levelised reserve over the weekly peaks of `load`) for the chronology's fleet: weeks[k] is
    the number of maintenance weeks of generators[k].  Returns the schedule as windows."""
    weeks = [int(w) for w in weeks]
    if len(weeks) != len(generators) or any(not 0 <= w <= n_weeks for w in weeks):
        raise ValueError(f"levelised_schedule: weeks needs one entry in [0, {n_weeks}] per generator")
    units = [hl1_planning.PlanningUnit(f"G{g.id}", g.capacity, g.for_rate, w) for g, w in zip(generators, weeks)]
    hl1_planning.schedule_maintenance(units, hl1_planning.weekly_peaks(load.hourly_load, n_weeks))
    return schedule_from_planning(units)


def run_sequential_maintenance(generators, load: hl1.LoadModel, schedules, n_years: int, *, chains: int = 1, start: str = "all_up",
                               seed: int = 1, scale: float = 1.0, shift: float = 0.0, engine=None) -> MaintenanceResult:
    """run_sequential_mc's chronology (same arguments, same chains under the same seed) under up to 8 maintenance schedules in one walk
    of the chains, against the load scale * load + shift.  Every schedule sees the same fleet history, so a schedule whose maintenance
    contains another's never loses less in any year, and two schedules may be differenced year by year (compare_schedules).  An empty
    schedule at the default scale and shift is run_sequential_mc bit for bit."""
    from . import api
    who = "run_sequential_maintenance"
    years, chains = hl1._seq_shape(who, n_years, chains, start)
    H = int(np.asarray(load.hourly_load).size)
    sch = _schedules(who, schedules, len(generators), H)
    _curve(who, load, scale, shift)
    eng = engine or api.default_engine()
    t0 = time.time()
    hl1._seq_model_load(eng, generators, load)
    n = len(sch)
    flat = [_abi.Hl1MaintWindow(j, int(w.unit), int(w.start_hour), int(w.hours)) for j, s in enumerate(sch) for w in s]
    arr = (_abi.Hl1MaintWindow * max(len(flat), 1))(*flat)
    eng._check(eng.L.relmc_hl1_maint_load(eng._h, n, len(flat), arr if flat else None), "relmc_hl1_maint_load")
    acc = (_abi.Hl1SeqAcc * n)()
    yr = np.zeros((n, years, 3))
    eng._check(eng.L.relmc_hl1_maint_seq(eng._h, int(seed), 0, chains, years // chains, hl1._SEQ_START[start], float(scale), float(shift), acc,
                                         yr.ctypes.data_as(C.POINTER(_abi.Hl1SeqYear))), "relmc_hl1_maint_seq")
    mean = lambda f: np.array([getattr(a, f) for a in acc]) / years
    yl, ye, yf = (np.ascontiguousarray(yr[:, :, q]) for q in range(3))
    return MaintenanceResult(sch, years, mean("sum_lole"), mean("sum_eue"), mean("sum_lolf"), hl1._se(yl), hl1._se(ye), hl1._se(yf), yl, ye, yf,
                             time.time() - t0)


def run_analytical_maintenance(generators, load: hl1.LoadModel, schedules, *, scale: float = 1.0, shift: float = 0.0,
                               step_size: float = 1.0) -> AnalyticalMaintenance:
    """The exact stationary counterpart: LOLE = sum over the hours of P(avail_h < L_h) and EUE the expected deficit likewise, where avail_h
    is the capacity of the units not on maintenance in hour h, each out with its forced outage rate.  The hours of the year are grouped by
    their maintenance set and every distinct set takes one COPT (hl1.run_analytical on the fleet without the set and the hours of the
    group), so a schedule without windows is hl1.run_analytical itself."""
    t0 = time.time()
    who = "run_analytical_maintenance"
    curve = _curve(who, load, scale, shift)
    sch = _schedules(who, schedules, len(generators), curve.size)
    lole, eue, ncopt = [], [], []
    for s in sch:
        on = maintenance_mask(s, len(generators), curve.size)
        sets, first, inv = np.unique(on, axis=0, return_index=True, return_inverse=True)
        inv = np.asarray(inv).reshape(-1)
        l = e = 0.0
        for i in np.argsort(first):                              # the groups in the order their first hour appears
            fleet = [g for k, g in enumerate(generators) if not sets[i, k]]
            r = hl1.run_analytical(fleet, hl1.LoadModel(curve[inv == i]), step_size=step_size)
            l += r.lole_hours_yr
            e += r.eue_mwh_yr
        lole.append(l); eue.append(e); ncopt.append(len(sets))
    return AnalyticalMaintenance(np.array(lole), np.array(eue), np.array(ncopt), time.time() - t0)


def compare_schedules(result: MaintenanceResult, base: int = 0) -> ScheduleComparison:
    """Every schedule minus schedule `base`: the differences of the indices, the standard error of the mean per-year difference (the
    schedules share the fleet history, so this is the error of the comparison), and beside it sqrt(se_j^2 + se_base^2), the error two
    independent runs would have."""
    n = len(result.schedules)
    if isinstance(base, bool) or not isinstance(base, (int, np.integer)) or not 0 <= base < n:
        raise ValueError(f"compare_schedules: base must be a schedule index in [0, {n}), not {base!r}")
    out = []
    for yr, se in ((result.year_lole, result.lole_se), (result.year_eue, result.eue_se), (result.year_lolf, result.lolf_se)):
        d = yr - yr[base][None, :]
        out.append((d.mean(axis=1), hl1._se(d), np.sqrt(se ** 2 + se[base] ** 2)))
    return ScheduleComparison(int(base), out[0][0], out[1][0], out[2][0], out[0][1], out[1][1], out[2][1], out[0][2], out[1][2], out[2][2])


def maintenance_report(result: MaintenanceResult, analytical: AnalyticalMaintenance = None, base: int = 0) -> str:
    """One row per schedule: its windows and unit-hours, LOLE, EUE and LOLF with standard errors, the paired LOLE difference to schedule
    `base`, and with `analytical` the exact LOLE / EUE beside them."""
    cmp_ = compare_schedules(result, base)
    rule = "=" * 42
    head = "%-8s | %-7s | %-10s | %-20s | %-21s | %-12s | %-22s" % ("Schedule", "Windows", "Unit-hours", "LOLE(h/yr) +- SE", "EUE(MWh/yr) +- SE",
                                                                    "LOLF(occ/yr)", "dLOLE vs %d +- SE" % base)
    if analytical is not None:
        head += " | %-10s | %-10s" % ("LOLE exact", "EUE exact")
    lines = [rule, "       MAINTENANCE SCHEDULE SUMMARY", rule, head, "-" * len(head)]
    for j, s in enumerate(result.schedules):
        row = "%-8d | %-7d | %-10d | %-9.4f +- %-7.4f | %-11.2f +- %-6.2f | %-12.4f | %-+10.4f +- %-8.4f" % (
            j, len(s), sum(w.hours for w in s), result.lole_hours_yr[j], result.lole_se[j], result.eue_mwh_yr[j], result.eue_se[j],
            result.lolf_occ_yr[j], cmp_.d_lole[j], cmp_.d_lole_se[j])
        if analytical is not None:
            row += " | %-10.4f | %-10.2f" % (analytical.lole_hours_yr[j], analytical.eue_mwh_yr[j])
        lines.append(row)
    lines.append("-" * len(head))
    return "\n".join(lines) + "\n"
