"""HL1 planning model: planned maintenance, energy-limited units (ELUs) and load forecast uncertainty (LFU).

Mirror of the reference's GeneratingAdequacy/ planning scripts:
  PlanningUnit                                 generating_adequacy_comprehensive.jl:10-23
  convolve_unit (hl1)                          :34-70      COPT step with capacity rounding, on the unit's effective q
  get_lfu_distribution()                       :76-80      the 7-step LFU of the analytic method
  weekly_peaks(load)                           generating_adequancy_comparative.jl:145
  schedule_maintenance(units, peaks)           comprehensive.jl:86-112   levelised reserve, stable tie order
  update_elu(units, load, step, sigma)         :118-175    one Gauss-Seidel pass of the ELU effective-q iteration
  run_detailed_analytical(units, load, pct)    tail_risk.jl:96-141 (comparative.jl:157-194)   weekly COPTs, hourly risk profile
  run_monte_carlo_simulation(units, load, pct, n_years)
                                               comparative.jl:15-120, tail_risk.jl:12-91 (MCvsMarkovProcess.jl:210-284 is the same
                                               loop), evaluated by the HIP library (relmc_hl1_plan_load / relmc_hl1_plan)
  tail_summary(values)                         the numeric content of tail_risk.jl:166-175's histogram
  comparison_report(analytical, mc)            comparative.jl:202-215
  toy_fleet() / toy_load(seed)                 comparative.jl:132-146
  rts24_planning_units()                       the 32 RTS-24 units with their maintenance weeks, no ELU

Deviations, all stated in DESIGN.md §6.11:
  * toy_load draws its noise with numpy, not with Julia's generator: the curve has the reference's shape, not its numbers.
  * The Monte Carlo draws are counter-based (include/relmc.h): Philox blocks per (year, hour), Box-Muller normals.
  * The analytic method evaluates weeks 1..52 only, as the reference does: hours past 52 * 168 = 8736 keep risk 0.
  * The analytic "installed capacity" is the last state of the rounded COPT grid, not the sum of the capacities (the reference's quirk).
  * Start week 0 means "not scheduled" (the reference only meets it for units with 0 maintenance weeks).
"""
from __future__ import annotations

import ctypes as C
import math
import time
from dataclasses import dataclass, field

import numpy as np

from . import _abi, case24, hl1

HOURS_PER_WEEK = 168
N_WEEKS = 52


@dataclass
class PlanningUnit:                   # comprehensive.jl:10-23
    name: str
    capacity: float
    for_rate: float                   # base forced outage rate
    maintenance_weeks: int = 0
    energy_limit: float = math.inf    # MWh per year; inf = not energy-limited
    effective_q: float | None = None  # the ELU iteration's adjusted q (starts at for_rate)
    scheduled_outage_start: int = 0   # 1-based week, 0 = none
    history_q: list = field(default_factory=list)

    def __post_init__(self):
        if self.effective_q is None:
            self.effective_q = self.for_rate
        if not self.history_q:
            self.history_q = [self.for_rate]

    @property
    def is_elu(self) -> bool:
        return self.energy_limit != math.inf

    def in_maintenance(self, week: int) -> bool:
        s = self.scheduled_outage_start
        return s >= 1 and s <= week < s + self.maintenance_weeks


@dataclass
class PlanningAnalyticalResult(hl1.ReliabilityResult):
    """run_detailed_analytical's result: hourly risk (P(loss) per hour, 0 past hour 8736), the final effective q of every unit and the
    q history of each ELU (one entry per iteration after the base FOR)."""
    hourly_risk: np.ndarray = field(default_factory=lambda: np.zeros(0))
    effective_q: np.ndarray = field(default_factory=lambda: np.zeros(0))
    history_q: dict = field(default_factory=dict)


@dataclass
class PlanningMCResult(hl1.ReliabilityResult):
    """run_monte_carlo_simulation's result: the reference's LOLE / EUE and 100-year running LOLE, plus loss events per year, the per-year
    arrays, the hourly loss probability (tail_risk.jl:81-88) and the MWh used per ELU per year ([n_years, n_elu], ELUs in unit order)."""
    lolf_occ_yr: float = 0.0
    year_lole: np.ndarray = field(default_factory=lambda: np.zeros(0))
    year_eue: np.ndarray = field(default_factory=lambda: np.zeros(0))
    year_lolf: np.ndarray = field(default_factory=lambda: np.zeros(0))
    hourly_loss_prob: np.ndarray = field(default_factory=lambda: np.zeros(0))
    elu_energy: np.ndarray = field(default_factory=lambda: np.zeros((0, 0)))
    elu_names: list = field(default_factory=list)


def toy_fleet() -> list:
    """The six units of comparative.jl:132-140: the hydro unit has 50 full-output hours of water."""
    return [PlanningUnit("Nuclear", 400.0, 0.02, 4), PlanningUnit("Coal_A", 300.0, 0.04, 3), PlanningUnit("Coal_B", 300.0, 0.04, 3),
            PlanningUnit("Gas", 150.0, 0.05, 2), PlanningUnit("Hydro_ELU", 200.0, 0.01, 2, 200.0 * 50.0),
            PlanningUnit("Old_56", 56.0, 0.10, 0)]


def toy_load(seed: int = 1, hours: int = 8760) -> np.ndarray:
    """750 + 300 sin((h - 2000) / 8760 * 2 pi) + 50 N(0, 1), floored at 0 (comparative.jl:142-144).  The noise comes from numpy's
    generator seeded with `seed`, not from Julia's: same shape, different numbers."""
    h = np.arange(1, hours + 1, dtype=np.float64)
    noise = np.random.default_rng(seed).standard_normal(hours)
    return np.maximum(0.0, 750.0 + 300.0 * np.sin((h - 2000.0) / 8760.0 * 2.0 * np.pi) + 50.0 * noise)


def rts24_planning_units() -> list:
    """The 32 RTS-24 units with case24_failrate()'s maintenance weeks and FOR = mttr / (mttf + mttr); none energy-limited."""
    d = case24.case24_failrate()
    return [PlanningUnit(f"G{g.id}", g.capacity, g.for_rate, int(round(d["genweeks"][g.id - 1])))
            for g in hl1.rts24_generators()]


def get_lfu_distribution() -> list:
    """The 7-step normal approximation (z in standard deviations, probability) of comprehensive.jl:76-80."""
    return [(-3.0, 0.006), (-2.0, 0.061), (-1.0, 0.242), (0.0, 0.382), (1.0, 0.242), (2.0, 0.061), (3.0, 0.006)]


def weekly_peaks(load, n_weeks: int = N_WEEKS) -> np.ndarray:
    """Maximum of hours (w-1)*168+1 .. min(w*168, H) for w = 1..n_weeks; a week with no hour of the curve has peak 0."""
    load = np.asarray(load, dtype=np.float64)
    out = np.zeros(n_weeks)
    for w in range(n_weeks):
        seg = load[w * HOURS_PER_WEEK:min((w + 1) * HOURS_PER_WEEK, load.size)]
        if seg.size:
            out[w] = seg.max()
    return out


def schedule_maintenance(units, peaks) -> list:
    """Levelised-reserve scheduling (comprehensive.jl:86-112), in place.  Units by capacity * weeks, descending (stable: equal keys keep
    their input order); each takes the earliest start week that maximises the minimum over its window of (available - peak) (strict >),
    and its capacity leaves that window.  Returns the start weeks in unit order."""
    peaks = np.asarray(peaks, dtype=np.float64)
    nw = peaks.size
    avail = np.full(nw, float(sum(u.capacity for u in units)))
    for u in sorted(units, key=lambda u: u.capacity * u.maintenance_weeks, reverse=True):
        m = int(u.maintenance_weeks)
        if m == 0:
            continue
        best, best_res = 1, -math.inf
        for s in range(1, nw - m + 2):
            res = float(np.min(avail[s - 1:s - 1 + m] - peaks[s - 1:s - 1 + m]))
            if res > best_res:
                best, best_res = s, res
        u.scheduled_outage_start = best
        avail[best - 1:best - 1 + m] -= u.capacity
    return [u.scheduled_outage_start for u in units]


def _copt(caps, qs, step_size: float) -> tuple:
    """COPT of the given units (probabilities on the grid k * step_size) and its "installed capacity" = the grid's last state."""
    probs = np.array([1.0])
    for c, q in zip(caps, qs):
        probs = hl1.convolve_unit(probs, c, q, step_size)
    return probs, (probs.size - 1) * step_size


def _expected_generation(probs, installed, step_size, unit_cap, load, sigma) -> float:
    """Expected MWh an ELU of `unit_cap` supplies over the curve under the 7-step LFU (comprehensive.jl:118-143)."""
    outage = np.arange(probs.size) * step_size
    total = 0.0
    for z, pz in get_lfu_distribution():
        thr = installed - (load + z * sigma)                        # reserve threshold per hour
        d = outage[None, :] - thr[:, None]
        term = np.where(d > 0.0, np.minimum(unit_cap, d), 0.0) @ probs
        total += float(np.sum(term * pz))
    return total


def update_elu(units, load, step_size: float, lfu_sigma_mw: float) -> bool:
    """One pass of comprehensive.jl:145-175 over the ELUs in unit order (Gauss-Seidel: later ELUs see the new q of earlier ones).
    The rest-of-system COPT ignores maintenance, as the reference does.  Returns whether some |dq| > 1e-5."""
    load = np.asarray(load, dtype=np.float64)
    changed = False
    for g in units:
        if not g.is_elu:
            continue
        rest = [u for u in units if u is not g]
        probs, installed = _copt([u.capacity for u in rest], [u.effective_q for u in rest], step_size)
        req = _expected_generation(probs, installed, step_size, g.capacity, load, lfu_sigma_mw)
        new_q = g.for_rate
        if req > g.energy_limit:
            new_q += (req - g.energy_limit) / (g.capacity * load.size)
        new_q = min(new_q, 1.0)
        if abs(new_q - g.effective_q) > 1e-5:
            g.effective_q = new_q
            changed = True
        g.history_q.append(new_q)
    return changed


def run_detailed_analytical(units, load, lfu_sigma_percent: float, step_size: float = 20.0,
                            elu_iterations: int = 5) -> PlanningAnalyticalResult:
    """tail_risk.jl:96-141: `elu_iterations` passes of update_elu (comparative.jl:157-159 runs 5 unconditionally), then for weeks 1..52 the
    COPT of the units not in maintenance (effective q) and risk_h = sum_z p_z P(outage > installed - (load_h + z sigma)).  LOLE = sum of the
    hourly risk.  EUE is the same sum of the expected deficit.  Hours past 52 * 168 are not evaluated (the reference's window)."""
    t0 = time.time()
    load = np.asarray(load, dtype=np.float64)
    sigma = float(load.max()) * (lfu_sigma_percent / 100.0)
    for _ in range(int(elu_iterations)):
        update_elu(units, load, step_size, sigma)
    risk = np.zeros(load.size)
    eue = 0.0
    for w in range(1, N_WEEKS + 1):
        h0, h1 = (w - 1) * HOURS_PER_WEEK, min(w * HOURS_PER_WEEK, load.size)
        if h0 >= h1:
            break
        week = [u for u in units if not u.in_maintenance(w)]
        probs, installed = _copt([u.capacity for u in week], [u.effective_q for u in week], step_size)
        outage = np.arange(probs.size) * step_size
        for z, pz in get_lfu_distribution():
            res = installed - (load[h0:h1] + z * sigma)
            d = outage[None, :] - res[:, None]
            risk[h0:h1] += ((d > 0.0) @ probs) * pz
            eue += float(np.sum((np.where(d > 0.0, d, 0.0) @ probs) * pz))
    hist = {u.name: list(u.history_q) for u in units if u.is_elu}
    return PlanningAnalyticalResult("Analytical (ELU)", float(risk.sum()), eue, time.time() - t0, hourly_risk=risk,
                                    effective_q=np.array([u.effective_q for u in units]), history_q=hist)


def _device_arrays(units):
    cap = np.ascontiguousarray([u.capacity for u in units], dtype=np.float64)
    forr = np.ascontiguousarray([u.for_rate for u in units], dtype=np.float64)
    start = np.ascontiguousarray([u.scheduled_outage_start for u in units], dtype=np.int32)
    weeks = np.ascontiguousarray([u.maintenance_weeks for u in units], dtype=np.int32)
    lim = np.ascontiguousarray([u.energy_limit for u in units], dtype=np.float64)
    return cap, forr, start, weeks, lim


def run_monte_carlo_simulation(units, load, lfu_sigma_percent: float, n_years: int, *, seed: int = 1,
                               engine=None) -> PlanningMCResult:
    """comparative.jl:15-120 / tail_risk.jl:12-91 on the GPU: n_years independent years, each starting with every ELU's energy at 0;
    maintenance from scheduled_outage_start, the *base* FOR for the draws, load_h + sigma Z with sigma = max(load) * pct / 100.
    convergence_history = running LOLE every 100 years (comparative.jl:114-116)."""
    from . import api
    n_years = int(n_years)
    if n_years < 1:
        raise ValueError(f"run_monte_carlo_simulation: n_years ({n_years}) must be positive")
    eng = engine or api.default_engine()
    L = eng.L
    t0 = time.time()
    hl = np.ascontiguousarray(load, dtype=np.float64)
    sigma = float(hl.max()) * (lfu_sigma_percent / 100.0)
    arrs = _device_arrays(units)
    key = tuple(a.tobytes() for a in arrs) + (hl.tobytes(), sigma)
    if getattr(eng, "_hl1_plan_loaded", None) != key:      # fleet and load curve stay on the device between calls on the same model
        cap, forr, start, weeks, lim = arrs
        eng._check(L.relmc_hl1_plan_load(eng._h, cap.size, cap.ctypes.data_as(_abi.c_double_p), forr.ctypes.data_as(_abi.c_double_p),
                                         start.ctypes.data_as(_abi.c_int32_p), weeks.ctypes.data_as(_abi.c_int32_p),
                                         lim.ctypes.data_as(_abi.c_double_p), hl.size, hl.ctypes.data_as(_abi.c_double_p), sigma),
                   "relmc_hl1_plan_load")
        eng._hl1_plan_loaded = key
    elus = [u.name for u in units if u.is_elu]
    acc = _abi.Hl1SeqAcc()
    yr = np.zeros((n_years, 3))
    hours = np.zeros(hl.size, dtype=np.int64)
    elu = np.zeros((n_years, len(elus)))
    eng._check(L.relmc_hl1_plan(eng._h, int(seed), 0, n_years, C.byref(acc), yr.ctypes.data_as(C.POINTER(_abi.Hl1SeqYear)),
                                hours.ctypes.data_as(_abi.c_int64_p), elu.ctypes.data_as(_abi.c_double_p) if elus else None),
               "relmc_hl1_plan")
    k = np.arange(100, n_years + 1, 100)
    history = np.cumsum(yr[:, 0])[k - 1] / k if k.size else np.zeros(0)
    return PlanningMCResult("Monte Carlo (ELU)", acc.sum_lole / n_years, acc.sum_eue / n_years, time.time() - t0, history,
                            lolf_occ_yr=acc.sum_lolf / n_years, year_lole=yr[:, 0].copy(), year_eue=yr[:, 1].copy(),
                            year_lolf=yr[:, 2].copy(), hourly_loss_prob=hours / n_years, elu_energy=elu, elu_names=elus)


def tail_summary(values, levels=(0.9, 0.95, 0.99)) -> dict:
    """Mean, standard deviation (n - 1, as Julia's std), the quantiles at `levels` (numpy's default linear rule = Julia's quantile) and the
    mean of the values at or beyond each quantile: the numbers behind tail_risk.jl's histogram of the annual outcomes."""
    v = np.asarray(values, dtype=np.float64)
    q = {float(a): float(np.quantile(v, a)) for a in levels}
    return {"mean": float(v.mean()), "std": float(v.std(ddof=1)) if v.size > 1 else 0.0, "quantile": q,
            "tail_mean": {a: float(v[v >= x].mean()) for a, x in q.items()}}


def comparison_report(analytical, mc) -> str:
    """The report of comparative.jl:202-215 (the plot is out of scope)."""
    a, m = analytical.lole_hours_yr, mc.lole_hours_yr
    rule = "-" * 50
    verdict = ("SUCCESS: The methods match closely! The Iterative Analytical method successfully approximated the complex ELU behavior."
               if abs(m - a) < 50.0 else
               "NOTICE: There is a gap. This highlights the 'Tail Risk' that Monte Carlo captures better than convolution.")
    return "\n".join(["", rule, "FINAL RESULTS COMPARISON", rule,
                      "Analytical LOLE (Iterative ELU): %.4f hours/year" % a,
                      "Monte Carlo LOLE (Sequential):   %.4f hours/year" % m,
                      "", "Conclusion:", verdict]) + "\n"
