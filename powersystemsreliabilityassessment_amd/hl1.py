"""HL1 (copper-sheet) generating-adequacy track — SURVEY.md §8f rank 1, BASELINE config 1.

Mirror of the reference's Julia module GeneratingAdequacy/PowerSystemAdequacy.jl:
  Generator / LoadModel / ReliabilityResult   (:20-52)
  run_analytical(gens, load; step_size)       (:113-163)  exact COPT convolution, host arithmetic (numpy)
  run_non_sequential_mc(gens, load, iterations)(:169-208)  Monte Carlo, evaluated by the HIP library
                                                            (relmc_hl1_load / relmc_hl1_nsq)
  run_sequential_mc(gens, load, years)         (:214-268)  chronological Monte Carlo on the GPU, with loss-of-load
                                                            frequency (relmc_hl1_seq_load / relmc_hl1_seq)
  compare_results(results)                     (:275-290)  the comparison table (text; no plot)
  run_sequential_events(gens, load, years)     the loss events of that chronology: durations, energies, peaks, histogram, event list
                                                            (relmc_hl1_seq_events)
  run_frequency_duration(gens, load_mw)        generating_adequacy_frequency.jl:53-186: the frequency-and-duration recursion (host)
  frequency_duration_report(analytical, events) LOLE / LOLF / LOLD of the two side by side (text)
  run_load_sweep(gens, load, years, levels)    an extension beyond the reference: one chronology against up to 16 load levels
                                                            (relmc_hl1_seq_sweep), and on it the planner's two questions,
  peak_load_carrying_capability / effective_load_carrying_capability, with analytical_load_sweep / analytical_plcc /
  analytical_elcc as their exact counterparts through run_analytical, and load_sweep_report for the table
`rts24_generators()` / `rts24_load()` give the IEEE RTS-79 fleet and the 8736-hour reference load
curve (Montecarlo_seq/anloducurve.m) whose exact answers are the published LOLE 9.3941 h/yr and
EUE 1176.29 MWh/yr.
"""
from __future__ import annotations

import ctypes as C
import time
from dataclasses import dataclass, field

import numpy as np

from . import _abi, case24, loadcurve


@dataclass
class Generator:                      # PowerSystemAdequacy.jl:20-37
    id: int
    capacity: float
    mttf: float
    mttr: float

    @property
    def for_rate(self) -> float:
        lam, mu = 1.0 / self.mttf, 1.0 / self.mttr
        return lam / (lam + mu)


@dataclass
class LoadModel:                      # :39-45
    hourly_load: np.ndarray

    @property
    def peak_load(self) -> float:
        return float(np.max(self.hourly_load))


@dataclass
class ReliabilityResult:              # :47-53
    method: str
    lole_hours_yr: float
    eue_mwh_yr: float
    computation_time: float
    convergence_history: np.ndarray = field(default_factory=lambda: np.zeros(0))


@dataclass
class SequentialReliabilityResult(ReliabilityResult):
    """run_sequential_mc's result: the reference's fields plus frequency / duration and the per-year indices (global year order,
    chain-major: the years of chain 0, then chain 1, ...)."""
    lolf_occ_yr: float = 0.0          # loss-of-load events per year
    lold_hours: float = float("nan")  # hours per event, LOLE / LOLF (NaN without an event)
    year_lole: np.ndarray = field(default_factory=lambda: np.zeros(0))
    year_eue: np.ndarray = field(default_factory=lambda: np.zeros(0))
    year_lolf: np.ndarray = field(default_factory=lambda: np.zeros(0))


def rts24_generators() -> list:
    d = case24.case24_failrate()
    return [Generator(i + 1, float(case24.GEN_PMAX[i]), float(d["genmttf"][i]), float(d["genmttr"][i]))
            for i in range(case24.GEN_PMAX.size) if case24.GEN_PMAX[i] > 0]     # 32 units (sync condenser has no capacity)


def rts24_load(hours: int = 8736) -> LoadModel:
    _, _, lf = loadcurve.anloducurve(hours)
    return LoadModel(2850.0 * lf)


def add_unit_convolution(probs: np.ndarray, unit: Generator, step_size: float) -> np.ndarray:
    """COPT recursion with capacity rounding split between neighbouring steps (:67-111).
    `probs[k]` = P(outage = k*step_size)."""
    return convolve_unit(probs, unit.capacity, unit.for_rate, step_size)


def convolve_unit(probs: np.ndarray, capacity: float, q: float, step_size: float) -> np.ndarray:
    """add_unit_convolution for a unit of `capacity` MW that is out with probability `q` (the planning model passes its effective q,
    generating_adequacy_comprehensive.jl:34-70)."""
    Cc = capacity
    p = 1.0 - q
    max_old = (probs.size - 1) * step_size if probs.size else 0.0
    n_new = int(np.ceil((max_old + Cc) / step_size)) + 1
    new = np.zeros(n_new)

    def shifted(k):            # get_prob(X - k*step) for all X
        out = np.zeros(n_new)
        if k < n_new:
            m = min(probs.size, n_new - k)
            out[k:k + m] = probs[:m]
        return out

    lower = int(np.floor(Cc / step_size))
    if abs(Cc - lower * step_size) < 1e-5:
        new = shifted(0) * p + shifted(lower) * q
    else:
        alpha = (Cc - lower * step_size) / step_size
        new = shifted(0) * p + shifted(lower) * (q * (1.0 - alpha)) + shifted(lower + 1) * (q * alpha)
    return new


def run_analytical(gens, load: LoadModel, step_size: float = 10.0) -> ReliabilityResult:
    """Exact (up to the capacity step) LOLE / EUE by convolution (:113-163)."""
    t0 = time.time()
    probs = np.array([1.0])
    for g in gens:
        probs = add_unit_convolution(probs, g, step_size)
    outage = np.arange(probs.size) * step_size
    installed = sum(g.capacity for g in gens)
    cum = np.cumsum(probs[::-1])[::-1]                         # P(outage >= X)
    tail_w = np.cumsum((outage * probs)[::-1])[::-1]           # sum_{k>=i} outage_k p_k
    lole = eue = 0.0
    for load_mw in np.asarray(load.hourly_load, dtype=float):
        reserve = installed - load_mw
        idx = int(np.floor(reserve / step_size)) + 1           # 0-based index of the first state with outage > reserve
        if 0 <= idx < probs.size:
            lole += cum[idx]
            eue += tail_w[idx] - reserve * cum[idx]
        elif idx < 0:
            lole += 1.0
            eue += (load_mw - installed) + float(outage @ probs)
    return ReliabilityResult("Analytical", lole, eue, time.time() - t0)


def run_non_sequential_mc(gens, load: LoadModel, iterations: int, *, seed: int = 1, engine=None) -> ReliabilityResult:
    """PowerSystemAdequacy.jl:169-208 on the GPU: one fleet state per iteration swept over the whole
    hourly load curve; convergence history = running LOLE every 100 iterations (:202-204)."""
    from . import api
    eng = engine or api.default_engine()
    L = eng.L
    L.relmc_hl1_load.argtypes = [C.c_void_p, C.c_int32, _abi.c_double_p, _abi.c_double_p, C.c_int32, _abi.c_double_p]
    L.relmc_hl1_nsq.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int64, C.POINTER(Hl1Acc), _abi.c_double_p, _abi.c_double_p]
    t0 = time.time()
    cap = np.ascontiguousarray([g.capacity for g in gens], dtype=np.float64)
    forr = np.ascontiguousarray([g.for_rate for g in gens], dtype=np.float64)
    hl = np.ascontiguousarray(load.hourly_load, dtype=np.float64)
    key = (cap.tobytes(), forr.tobytes(), hl.tobytes())
    if getattr(eng, "_hl1_loaded", None) != key:           # the fleet and the sorted load curve stay on the device between calls on the same model
        eng._check(L.relmc_hl1_load(eng._h, cap.size, cap.ctypes.data_as(_abi.c_double_p), forr.ctypes.data_as(_abi.c_double_p),
                                    hl.size, hl.ctypes.data_as(_abi.c_double_p)), "relmc_hl1_load")
        eng._hl1_loaded = key
    acc = Hl1Acc()
    it_lole = np.zeros(iterations)
    eng._check(L.relmc_hl1_nsq(eng._h, int(seed), 0, int(iterations), C.byref(acc), it_lole.ctypes.data_as(_abi.c_double_p), None),
               "relmc_hl1_nsq")
    k = np.arange(100, iterations + 1, 100)
    history = np.cumsum(it_lole)[k - 1] / k if k.size else np.zeros(0)
    return ReliabilityResult("Non-Sequential MC", acc.sum_lole / iterations, acc.sum_eue / iterations, time.time() - t0, history)


_SEQ_START = {"all_up": _abi.HL1_START_ALL_UP, "stationary": _abi.HL1_START_STATIONARY}


def _seq_model_load(eng, gens, load: LoadModel) -> None:
    """relmc_hl1_seq_load, unless this fleet and load curve are already on the device (they stay there between calls on the same model)."""
    L = eng.L
    cap = np.ascontiguousarray([g.capacity for g in gens], dtype=np.float64)
    mttf = np.ascontiguousarray([g.mttf for g in gens], dtype=np.float64)
    mttr = np.ascontiguousarray([g.mttr for g in gens], dtype=np.float64)
    hl = np.ascontiguousarray(load.hourly_load, dtype=np.float64)
    key = (cap.tobytes(), mttf.tobytes(), mttr.tobytes(), hl.tobytes())
    if getattr(eng, "_hl1_seq_loaded", None) != key:
        eng._check(L.relmc_hl1_seq_load(eng._h, cap.size, cap.ctypes.data_as(_abi.c_double_p), mttf.ctypes.data_as(_abi.c_double_p),
                                        mttr.ctypes.data_as(_abi.c_double_p), hl.size, hl.ctypes.data_as(_abi.c_double_p)),
                   "relmc_hl1_seq_load")
        eng._hl1_seq_loaded = key


def run_sequential_mc(gens, load: LoadModel, years: int, *, seed: int = 1, chains: int = 1, start: str = "all_up",
                      engine=None) -> SequentialReliabilityResult:
    """PowerSystemAdequacy.jl:214-268 on the GPU: `chains` independent chronological chains of years // chains consecutive years each
    (the fleet state carries over from year to year inside a chain).  The defaults are the reference's shape: one chain, every unit UP
    at the start.  start="stationary" draws each unit's start state from its stationary distribution, so that short chains run in
    parallel are unbiased.  convergence_history = running LOLE every 10 years (:263-265)."""
    from . import api
    years, chains = int(years), int(chains)
    if years < 1 or chains < 1 or years % chains:
        raise ValueError(f"run_sequential_mc: years ({years}) must be a positive multiple of chains ({chains})")
    if start not in _SEQ_START:
        raise ValueError(f"run_sequential_mc: start must be one of {sorted(_SEQ_START)}, not {start!r}")
    eng = engine or api.default_engine()
    L = eng.L
    t0 = time.time()
    _seq_model_load(eng, gens, load)
    acc = _abi.Hl1SeqAcc()
    yr = np.zeros((years, 3))
    eng._check(L.relmc_hl1_seq(eng._h, int(seed), 0, chains, years // chains, _SEQ_START[start], C.byref(acc),
                               yr.ctypes.data_as(C.POINTER(_abi.Hl1SeqYear))), "relmc_hl1_seq")
    k = np.arange(10, years + 1, 10)
    history = np.cumsum(yr[:, 0])[k - 1] / k if k.size else np.zeros(0)
    lole, eue, lolf = acc.sum_lole / years, acc.sum_eue / years, acc.sum_lolf / years
    return SequentialReliabilityResult("Sequential MC", lole, eue, time.time() - t0, history, lolf_occ_yr=lolf,
                                       lold_hours=lole / lolf if lolf > 0 else float("nan"),
                                       year_lole=yr[:, 0].copy(), year_eue=yr[:, 1].copy(), year_lolf=yr[:, 2].copy())


def compare_results(results) -> str:
    """The method comparison table of :275-290 (the reference prints it and plots the convergence histories; plots are out of scope)."""
    rule = "=" * 42
    lines = [rule, "       METHOD COMPARISON SUMMARY", rule,
             "%-20s | %-10s | %-10s | %-10s" % ("Method", "LOLE(h/yr)", "EUE(MWh)", "Time(s)"), "-" * 60]
    lines += ["%-20s | %-10.4f | %-10.2f | %-10.4f" % (r.method, r.lole_hours_yr, r.eue_mwh_yr, r.computation_time) for r in results]
    lines.append("-" * 60)
    return "\n".join(lines) + "\n"


# ---- load sweep on one chronology: risk curves, PLCC and unit ELCC (an extension beyond the reference) --------------------------------
@dataclass(frozen=True)
class SweepLevel:
    """One level of a load sweep: the load curve scale * load + shift (MW), against the whole fleet or, with withheld=True, against the
    fleet without the sweep's withheld units."""
    scale: float = 1.0
    shift: float = 0.0
    withheld: bool = False


@dataclass
class LoadSweepResult:
    """run_load_sweep's result: index j is level j.  The standard errors are over the simulated years (NaN with a single year)."""
    levels: list
    withheld_units: tuple
    years: int
    lole_hours_yr: np.ndarray
    eue_mwh_yr: np.ndarray
    lolf_occ_yr: np.ndarray
    lole_se: np.ndarray
    eue_se: np.ndarray
    lolf_se: np.ndarray
    year_lole: np.ndarray             # [n_levels, years], chain-major as run_sequential_mc's
    year_eue: np.ndarray
    year_lolf: np.ndarray
    computation_time: float

    def result(self, j: int) -> SequentialReliabilityResult:
        """Level j as run_sequential_mc would report it (compare_results takes it)."""
        lv = self.levels[j]
        lole, eue, lolf = float(self.lole_hours_yr[j]), float(self.eue_mwh_yr[j]), float(self.lolf_occ_yr[j])
        k = np.arange(10, self.years + 1, 10)
        history = np.cumsum(self.year_lole[j])[k - 1] / k if k.size else np.zeros(0)
        name = "Sweep %gx%+g%s" % (lv.scale, lv.shift, " w/o" if lv.withheld else "")
        return SequentialReliabilityResult(name, lole, eue, self.computation_time, history, lolf_occ_yr=lolf,
                                           lold_hours=lole / lolf if lolf > 0 else float("nan"), year_lole=self.year_lole[j].copy(),
                                           year_eue=self.year_eue[j].copy(), year_lolf=self.year_lolf[j].copy())


@dataclass
class AnalyticalLoadSweep:
    """analytical_load_sweep's result: run_analytical's LOLE and EUE per level."""
    levels: list
    withheld_units: tuple
    lole_hours_yr: np.ndarray
    eue_mwh_yr: np.ndarray
    computation_time: float


def _sweep_levels(who: str, levels, n_units: int, withheld_units) -> tuple:
    """The checks of a sweep's levels and withheld units that need no device; returns (list of SweepLevel, sorted tuple of unit indices)."""
    lv = [x if isinstance(x, SweepLevel) else SweepLevel(*x) for x in levels]
    if not 1 <= len(lv) <= _abi.HL1_SWEEP_MAX_LEVELS:
        raise ValueError(f"{who}: between 1 and {_abi.HL1_SWEEP_MAX_LEVELS} levels, not {len(lv)}")
    for j, x in enumerate(lv):
        if not (np.isfinite(x.scale) and np.isfinite(x.shift)):
            raise ValueError(f"{who}: scale / shift of level {j} not finite")
    wh = [int(k) for k in withheld_units]
    if len(set(wh)) != len(wh) or any(not 0 <= k < n_units for k in wh):
        raise ValueError(f"{who}: withheld_units must be distinct unit indices in [0, {n_units}), not {list(withheld_units)}")
    if not wh and any(x.withheld for x in lv):
        raise ValueError(f"{who}: a level with withheld=True needs withheld_units")
    return lv, tuple(sorted(wh))


def _seq_shape(who: str, years, chains, start) -> tuple:
    years, chains = int(years), int(chains)
    if years < 1 or chains < 1 or years % chains:
        raise ValueError(f"{who}: years ({years}) must be a positive multiple of chains ({chains})")
    if start not in _SEQ_START:
        raise ValueError(f"{who}: start must be one of {sorted(_SEQ_START)}, not {start!r}")
    return years, chains


def _se(x: np.ndarray) -> np.ndarray:
    """Standard error of the mean along the last axis (NaN with one value)."""
    n = x.shape[-1]
    return x.std(axis=-1, ddof=1) / np.sqrt(n) if n > 1 else np.full(x.shape[:-1], np.nan)


def run_load_sweep(gens, load: LoadModel, years: int, levels, *, withheld_units=(), seed: int = 1, chains: int = 1, start: str = "all_up",
                   engine=None) -> LoadSweepResult:
    """run_sequential_mc's chronology (same arguments, same chains under the same seed) against up to 16 load levels in one walk of the
    chains.  Level j sees the load scale_j * load + shift_j and, with withheld=True, the fleet without the units `withheld_units`
    (0-based indices into gens).  Every level sees the same fleet history, so the sampled LOLE and EUE are exactly monotone in a load
    shift and two levels may be differenced year by year.  Level SweepLevel() is run_sequential_mc bit for bit."""
    from . import api
    years, chains = _seq_shape("run_load_sweep", years, chains, start)
    lv, wh = _sweep_levels("run_load_sweep", levels, len(gens), withheld_units)
    eng = engine or api.default_engine()
    t0 = time.time()
    _seq_model_load(eng, gens, load)
    n = len(lv)
    arr = (_abi.Hl1SweepLevel * n)(*[_abi.Hl1SweepLevel(float(x.scale), float(x.shift), 1 if x.withheld else 0, 0) for x in lv])
    mask = None
    if wh:
        mask = (C.c_uint32 * 4)()
        for k in wh:
            mask[k >> 5] |= 1 << (k & 31)
    acc = (_abi.Hl1SeqAcc * n)()
    yr = np.zeros((n, years, 3))
    eng._check(eng.L.relmc_hl1_seq_sweep(eng._h, int(seed), 0, chains, years // chains, _SEQ_START[start], n, arr, mask, acc,
                                         yr.ctypes.data_as(C.POINTER(_abi.Hl1SeqYear))), "relmc_hl1_seq_sweep")
    mean = lambda f: np.array([getattr(a, f) for a in acc]) / years
    yl, ye, yf = (np.ascontiguousarray(yr[:, :, q]) for q in range(3))
    return LoadSweepResult(lv, wh, years, mean("sum_lole"), mean("sum_eue"), mean("sum_lolf"), _se(yl), _se(ye), _se(yf), yl, ye, yf,
                           time.time() - t0)


def _level_model(gens, load: LoadModel, lv: SweepLevel, wh) -> tuple:
    """The fleet and the load curve of one level, for run_analytical (the kernel rounds scale * load + shift the same way)."""
    fleet = [g for k, g in enumerate(gens) if not (lv.withheld and k in wh)]
    return fleet, LoadModel(lv.scale * np.asarray(load.hourly_load, dtype=float) + lv.shift)


def analytical_load_sweep(gens, load: LoadModel, levels, withheld_units=(), step_size: float = 1.0) -> AnalyticalLoadSweep:
    """The exact LOLE / EUE of every level of a sweep, through run_analytical on the level's curve and fleet."""
    t0 = time.time()
    lv, wh = _sweep_levels("analytical_load_sweep", levels, len(gens), withheld_units)
    res = [run_analytical(*_level_model(gens, load, x, wh), step_size=step_size) for x in lv]
    return AnalyticalLoadSweep(lv, wh, np.array([r.lole_hours_yr for r in res]), np.array([r.eue_mwh_yr for r in res]), time.time() - t0)


_SWEEP_METRIC = {"lole": "lole_hours_yr", "eue": "eue_mwh_yr"}
_SWEEP_MODE = {"shift": lambda x: SweepLevel(1.0, float(x)), "scale": lambda x: SweepLevel(float(x), 0.0)}


def _search_args(who: str, metric, mode, bracket, rounds) -> tuple:
    if metric not in _SWEEP_METRIC:
        raise ValueError(f"{who}: metric must be one of {sorted(_SWEEP_METRIC)}, not {metric!r}")
    if mode not in _SWEEP_MODE:
        raise ValueError(f"{who}: mode must be one of {sorted(_SWEEP_MODE)}, not {mode!r}")
    lo, hi = (float(b) for b in bracket)
    if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi):
        raise ValueError(f"{who}: bracket must be finite and ascending, not {tuple(bracket)}")
    if int(rounds) < 1:
        raise ValueError(f"{who}: rounds must be at least 1")
    return lo, hi, int(rounds)


def _bisect(f, target: float, lo: float, hi: float, tol: float, hi_is_bound: bool, who: str) -> float:
    """The largest x in [lo, hi] with f(x) <= target, for a non-decreasing f (run_analytical's LOLE is a staircase in the load)."""
    if f(lo) > target:
        raise ValueError(f"{who}: the target lies below the bracket")
    if f(hi) <= target:
        if hi_is_bound:
            return hi
        raise ValueError(f"{who}: the target lies above the bracket")
    while hi - lo > tol:
        mid = 0.5 * (lo + hi)
        if f(mid) <= target:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def analytical_plcc(gens, load: LoadModel, target: float, *, metric: str = "lole", mode: str = "shift", bracket, step_size: float = 1.0,
                    tol: float = 1e-6) -> float:
    """Peak load carrying capability by bisection on run_analytical: the largest load shift (MW; mode="scale": the largest scale factor)
    inside `bracket` at which the metric does not exceed `target`.  ValueError if the target lies outside the bracket."""
    lo, hi, _ = _search_args("analytical_plcc", metric, mode, bracket, 1)
    f = lambda x: getattr(run_analytical(*_level_model(gens, load, _SWEEP_MODE[mode](x), ()), step_size=step_size), _SWEEP_METRIC[metric])
    return _bisect(f, float(target), lo, hi, tol, False, "analytical_plcc")


def analytical_elcc(gens, load: LoadModel, units, *, metric: str = "lole", bracket=None, step_size: float = 1.0, tol: float = 1e-6) -> float:
    """Effective load carrying capability of the units `units` (0-based indices into gens) by bisection on run_analytical: the largest
    load shift (MW) at which the whole fleet is no riskier than the fleet without the units at the unshifted load.  The default bracket
    is (0, the units' capacity): units that never fail are worth exactly their capacity, which is then returned."""
    _, wh = _sweep_levels("analytical_elcc", [SweepLevel(withheld=True)], len(gens), units)
    if not wh:
        raise ValueError("analytical_elcc: no unit given")
    default = bracket is None
    lo, hi, _ = _search_args("analytical_elcc", metric, "shift", (0.0, sum(gens[k].capacity for k in wh)) if default else bracket, 1)
    attr = _SWEEP_METRIC[metric]
    target = getattr(run_analytical(*_level_model(gens, load, SweepLevel(withheld=True), wh), step_size=step_size), attr)
    f = lambda x: getattr(run_analytical(gens, LoadModel(np.asarray(load.hourly_load, dtype=float) + x), step_size=step_size), attr)
    return _bisect(f, target, lo, hi, tol, default, "analytical_elcc")


@dataclass
class CarryingCapabilityResult:
    """The result of peak_load_carrying_capability / effective_load_carrying_capability.  `value` is the load shift in MW (the scale factor
    with mode="scale") at which the sampled metric meets the target, interpolated linearly inside the final pair of levels."""
    method: str
    metric: str
    mode: str
    value: float
    std_error: float                  # delta method: the standard error of the metric (difference) over the local slope
    pair: tuple                       # the final pair of levels (lower, upper) ...
    pair_metric: tuple                # ... and the sampled metric at them
    target: float                     # the metric to meet (ELCC: the fleet without the units, at the unshifted load)
    years: int
    rounds: int
    computation_time: float
    target_year: list = field(default_factory=list)    # ELCC: the per-year metric of the target level, one array per round


def _pick_pair(who: str, m: np.ndarray, target: float) -> int:
    """Index i of the adjacent pair (i, i + 1) of the non-decreasing m that brackets the target."""
    if not m[0] <= target <= m[-1]:
        raise ValueError(f"{who}: the target {target:g} lies outside the bracket (the metric runs from {m[0]:g} to {m[-1]:g} over it)")
    return min(int(np.searchsorted(m, target, side="right")) - 1, m.size - 2)


def _interpolate(x: np.ndarray, m: np.ndarray, i: int, target: float) -> tuple:
    """(value, weight of the upper level, slope) of the linear interpolation inside the pair (i, i + 1)."""
    dm, dx = m[i + 1] - m[i], x[i + 1] - x[i]
    t = (target - m[i]) / dm if dm > 0 else 0.0
    return float(x[i] + t * dx), float(t), float(dm / dx)


def peak_load_carrying_capability(gens, load: LoadModel, target: float, years: int, *, metric: str = "lole", mode: str = "shift", bracket,
                                  rounds: int = 3, seed: int = 1, chains: int = 1, start: str = "all_up", engine=None) -> CarryingCapabilityResult:
    """How much load the fleet carries at the risk `target` (LOLE in h/yr or EUE in MWh/yr): the load shift in MW (mode="scale": the factor
    on the load curve) at which the sampled metric meets the target.  Each round sweeps 16 equally spaced levels over the bracket under
    the same seed -- the sampled metric is then exactly monotone along them -- and keeps the adjacent pair that brackets the target; the
    last pair is interpolated linearly.  ValueError if the target lies outside the bracket."""
    who = "peak_load_carrying_capability"
    years, chains = _seq_shape(who, years, chains, start)
    lo, hi, rounds = _search_args(who, metric, mode, bracket, rounds)
    t0 = time.time()
    target = float(target)
    for _ in range(rounds):
        x = np.linspace(lo, hi, _abi.HL1_SWEEP_MAX_LEVELS)
        sw = run_load_sweep(gens, load, years, [_SWEEP_MODE[mode](v) for v in x], seed=seed, chains=chains, start=start, engine=engine)
        m = getattr(sw, _SWEEP_METRIC[metric])
        i = _pick_pair(who, m, target)
        lo, hi = float(x[i]), float(x[i + 1])
    value, t, slope = _interpolate(x, m, i, target)
    se_m = getattr(sw, metric + "_se")[i + 1 if t > 0.5 else i]
    return CarryingCapabilityResult("Sequential MC sweep", metric, mode, value, float(se_m / slope) if slope > 0 else float("inf"), (lo, hi),
                                    (float(m[i]), float(m[i + 1])), target, years, rounds, time.time() - t0)


def effective_load_carrying_capability(gens, load: LoadModel, units, years: int, *, metric: str = "lole", bracket=None, rounds: int = 3,
                                       seed: int = 1, chains: int = 1, start: str = "all_up", engine=None) -> CarryingCapabilityResult:
    """What the units `units` (0-based indices into gens) are worth in load: the load shift in MW after which the whole fleet is as risky
    as the fleet without them at the unshifted load.  The search of peak_load_carrying_capability with 15 shifted levels of the whole
    fleet and one level of the fleet without the units per round; that level is the target and is bitwise the same in every round.  Both
    fleets see the same draws, so the standard error comes from the per-year paired differences between the interpolated pair and the
    target level, over the slope.  The default bracket is (0, the units' capacity)."""
    who = "effective_load_carrying_capability"
    years, chains = _seq_shape(who, years, chains, start)
    _, wh = _sweep_levels(who, [SweepLevel(withheld=True)], len(gens), units)
    if not wh:
        raise ValueError(f"{who}: no unit given")
    lo, hi, rounds = _search_args(who, metric, "shift", (0.0, sum(gens[k].capacity for k in wh)) if bracket is None else bracket, rounds)
    t0 = time.time()
    n = _abi.HL1_SWEEP_MAX_LEVELS - 1
    per_year = "year_" + metric
    target_year = []
    for _ in range(rounds):
        x = np.linspace(lo, hi, n)
        sw = run_load_sweep(gens, load, years, [SweepLevel(1.0, float(v)) for v in x] + [SweepLevel(withheld=True)], withheld_units=wh,
                            seed=seed, chains=chains, start=start, engine=engine)
        m, target = getattr(sw, _SWEEP_METRIC[metric])[:n], float(getattr(sw, _SWEEP_METRIC[metric])[n])
        target_year.append(getattr(sw, per_year)[n].copy())
        i = _pick_pair(who, m, target)
        lo, hi = float(x[i]), float(x[i + 1])
    value, t, slope = _interpolate(x, m, i, target)
    yr = getattr(sw, per_year)
    se_d = float(_se((1.0 - t) * yr[i] + t * yr[i + 1] - yr[n]))
    return CarryingCapabilityResult("Sequential MC sweep", metric, "shift", value, se_d / slope if slope > 0 else float("inf"), (lo, hi),
                                    (float(m[i]), float(m[i + 1])), target, years, rounds, time.time() - t0, target_year)


def load_sweep_report(sweep: LoadSweepResult, analytical: AnalyticalLoadSweep = None) -> str:
    """The levels of a sweep as a text table in compare_results' style, beside the analytic values if given."""
    rule = "=" * 42
    head = "%-5s | %-8s | %-10s | %-5s | %-20s | %-22s | %-12s" % ("Level", "Scale", "Shift(MW)", "Fleet", "LOLE(h/yr) +- SE", "EUE(MWh/yr) +- SE", "LOLF(occ/yr)")
    if analytical is not None:
        head += " | %-10s | %-10s" % ("LOLE exact", "EUE exact")
    lines = [rule, "          LOAD SWEEP SUMMARY", rule, head, "-" * len(head)]
    for j, lv in enumerate(sweep.levels):
        ln = "%-5d | %-8.4f | %-10.2f | %-5s | %-9.4f +- %-7.4f | %-11.2f +- %-7.2f | %-12.4f" % (
            j, lv.scale, lv.shift, "w/o" if lv.withheld else "all", sweep.lole_hours_yr[j], sweep.lole_se[j], sweep.eue_mwh_yr[j],
            sweep.eue_se[j], sweep.lolf_occ_yr[j])
        if analytical is not None:
            ln += " | %-10.4f | %-10.2f" % (analytical.lole_hours_yr[j], analytical.eue_mwh_yr[j])
        lines.append(ln)
    lines.append("-" * len(head))
    if sweep.withheld_units:
        lines.append("w/o: the fleet without units %s" % list(sweep.withheld_units))
    return "\n".join(lines) + "\n"


EVENT_DTYPE = np.dtype(_abi.Hl1Event)     # the structured view of relmc_hl1_event: chain, start_step, duration, energy_mwh, peak_mw


@dataclass
class LossEventResult:
    """run_sequential_events' result.  A loss event is a maximal run of consecutive loss hours of a chain (it may cross a year boundary;
    one that is still open at the chain's last hour ends there and counts as censored)."""
    method: str
    years: int
    n_events: int
    lole_hours_yr: float              # sum of the durations / years (= run_sequential_mc's LOLE)
    eue_mwh_yr: float                 # sum of the energies / years
    lolf_occ_yr: float                # events per year (= run_sequential_mc's LOLF)
    lold_hours: float                 # hours per event, sum of the durations / events (NaN without an event)
    mean_energy_mwh: float            # MWh per event (NaN without an event)
    max_duration: int
    max_energy_mwh: float
    max_peak_mw: float
    censored: int
    computation_time: float
    duration_hist: np.ndarray = field(default_factory=lambda: np.zeros(0, dtype=np.int64))   # [d - 1] = events of d hours, last bin: that long or longer
    events: np.ndarray = field(default_factory=lambda: np.zeros(0, dtype=EVENT_DTYPE))       # the first max_events events, (chain, start_step) order

    def duration_quantile(self, p: float) -> float:
        """Smallest duration d (hours) with P(D <= d) >= p, read off the histogram; NaN if it falls into the overflow bin (or there is no event)."""
        if not 0.0 <= p <= 1.0:
            raise ValueError(f"duration_quantile: p must lie in [0, 1], not {p}")
        total = int(self.duration_hist.sum())
        if total == 0:
            return float("nan")
        d = int(np.searchsorted(np.cumsum(self.duration_hist), p * total, side="left"))      # 0-based bin
        return float("nan") if d >= self.duration_hist.size - 1 else float(max(d, 0) + 1)


def run_sequential_events(gens, load: LoadModel, years: int, *, seed: int = 1, chains: int = 1, start: str = "all_up",
                          duration_bins: int = 168, max_events: int = 0, engine=None) -> LossEventResult:
    """The loss events of run_sequential_mc's chronology (same arguments, same chains under the same seed): how often interruptions
    occur, how long they last, their energy and peak.  duration_hist has duration_bins bins (the last one counts that many hours or
    more); `events` holds the first max_events events."""
    from . import api
    years, chains, duration_bins, max_events = int(years), int(chains), int(duration_bins), int(max_events)
    if years < 1 or chains < 1 or years % chains:
        raise ValueError(f"run_sequential_events: years ({years}) must be a positive multiple of chains ({chains})")
    if start not in _SEQ_START:
        raise ValueError(f"run_sequential_events: start must be one of {sorted(_SEQ_START)}, not {start!r}")
    if not 1 <= duration_bins <= 4096 or max_events < 0:
        raise ValueError("run_sequential_events: duration_bins must lie in [1, 4096] and max_events must not be negative")
    eng = engine or api.default_engine()
    t0 = time.time()
    _seq_model_load(eng, gens, load)
    acc = _abi.Hl1EventAcc()
    hist = np.zeros(duration_bins, dtype=np.int64)
    ev = np.zeros(max_events, dtype=EVENT_DTYPE)
    eng._check(eng.L.relmc_hl1_seq_events(eng._h, int(seed), 0, chains, years // chains, _SEQ_START[start], C.byref(acc), duration_bins,
                                          hist.ctypes.data_as(_abi.c_int64_p), max_events,
                                          ev.ctypes.data_as(C.POINTER(_abi.Hl1Event)) if max_events else None), "relmc_hl1_seq_events")
    n = acc.events
    nan = float("nan")
    return LossEventResult("Sequential MC events", years, n, acc.sum_dur / years, acc.sum_energy / years, n / years,
                           acc.sum_dur / n if n else nan, acc.sum_energy / n if n else nan, acc.max_dur, acc.max_energy, acc.max_peak,
                           acc.censored, time.time() - t0, hist, ev[:min(n, max_events)])


@dataclass
class FrequencyDurationResult:
    """run_frequency_duration's result: the indices at one load level and the cumulative table (P and F of outage >= level)."""
    method: str
    lole_hours_yr: float
    lolf_occ_yr: float
    lold_hours: float                 # LOLE / LOLF (NaN when LOLF is 0)
    computation_time: float
    levels: np.ndarray = field(default_factory=lambda: np.zeros(0))
    cum_prob: np.ndarray = field(default_factory=lambda: np.zeros(0))
    cum_freq: np.ndarray = field(default_factory=lambda: np.zeros(0))


def run_frequency_duration(gens, load_mw: float, step_size: float = 1.0) -> FrequencyDurationResult:
    """The frequency-and-duration recursion of generating_adequacy_frequency.jl (recursion :110-128, boundary rule :76-98, evaluation
    :155-186) at one load level, without the printing.  Per unit lambda = 8760 / mttf and mu = 8760 / mttr per year, q = lambda / (lambda + mu),
    p = 1 - q, and over the outage levels X = 0, step, 2 step, ...:
        P_new(X) = p P(X) + q P(X - C)
        F_new(X) = p F(X) + q F(X - C) + lambda p (P(X - C) - P(X))
    with P = 1, F = 0 below level 0 and P = F = 0 above the largest outage.  LOLE = 8760 P, LOLF = F and LOLD = LOLE / LOLF at the first
    level above the reserve (installed capacity - load).  The reference fixes the step at 1 MW; here a capacity that is not a multiple of
    step_size raises ValueError.
    This is the continuous-time answer.  The chronology of run_sequential_mc / run_sequential_events samples the fleet at integer hours:
    an outage that contains no integer hour is never seen and two events less than an hour apart merge, so its LOLF lies somewhat below
    this one (tests/tools/hl1_seq_model.small_fleet_stationary gives the exact sampled-chain frequency of a small fleet)."""
    t0 = time.time()
    if not step_size > 0:
        raise ValueError("run_frequency_duration: step_size must be positive")
    P, F = np.array([1.0]), np.array([0.0])
    installed = 0.0
    for g in gens:
        c = int(round(g.capacity / step_size))
        if c < 0 or abs(g.capacity - c * step_size) > 1e-9 * max(1.0, abs(g.capacity)):
            raise ValueError(f"run_frequency_duration: capacity {g.capacity} MW of unit {g.id} is not a multiple of the step {step_size} MW")
        lam, mu = 8760.0 / g.mttf, 8760.0 / g.mttr
        q = lam / (lam + mu)
        p = 1.0 - q
        P0, F0 = np.concatenate([P, np.zeros(c)]), np.concatenate([F, np.zeros(c)])       # old P(X), F(X): 0 above the old maximum
        Pc, Fc = np.concatenate([np.ones(c), P]), np.concatenate([np.zeros(c), F])        # old P(X - C), F(X - C): 1 and 0 below level 0
        P, F = p * P0 + q * Pc, p * F0 + q * Fc + lam * p * (Pc - P0)
        installed += g.capacity
    levels = np.arange(P.size) * step_size
    reserve = installed - float(load_mw)
    idx = int(np.searchsorted(levels, reserve, side="right"))      # first level > reserve
    lole, lolf = (8760.0 * float(P[idx]), float(F[idx])) if idx < P.size else (0.0, 0.0)
    return FrequencyDurationResult("Frequency & Duration", lole, lolf, lole / lolf if lolf > 0 else float("nan"), time.time() - t0,
                                   levels, P, F)


def frequency_duration_report(analytical: FrequencyDurationResult, events: LossEventResult) -> str:
    """LOLE / LOLF / LOLD of the analytic recursion and of the chronology's events side by side, in compare_results' style."""
    rule = "=" * 42
    lines = [rule, "     FREQUENCY & DURATION SUMMARY", rule,
             "%-20s | %-10s | %-12s | %-10s" % ("Method", "LOLE(h/yr)", "LOLF(occ/yr)", "LOLD(h)"), "-" * 62]
    lines += ["%-20s | %-10.4f | %-12.4f | %-10.4f" % (r.method, r.lole_hours_yr, r.lolf_occ_yr, r.lold_hours) for r in (analytical, events)]
    lines.append("-" * 62)
    return "\n".join(lines) + "\n"


class Hl1Acc(C.Structure):
    _fields_ = [("n", C.c_int64), ("sum_lole", C.c_double), ("sum_eue", C.c_double),
                ("sum_lole2", C.c_double), ("sum_eue2", C.c_double)]
