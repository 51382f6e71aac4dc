"""Weather-dependent forced outage rates on the HL1 sequential chronology — an extension beyond the reference, whose units fail at a
constant rate (PowerSystemAdequacy.jl:214-268).

Thermal units fail more often in the cold snap or heat wave that also drives the peak load.  An OutageStress library goes with the
WeatherYears library of hl1_variable.py: for every weather year, outage class and hour a multiplier on the failure rate 1 / mttf of the
units of that class.  Every chain year of a run draws a weather year, which now sets the load, the resources and the failure rates of
the same hours; repairs are unchanged (relmc_hl1_stress_load, relmc_hl1_stress_seq; the rules are written out in include/relmc.h).

  OutageStress(fail_mult[n_weather, n_classes, H], unit_class[n_units], names=())   the library; unit_class -1: the unit ignores the weather
  synthetic_stress(weather, load, gens, ...)                                        an illustrative library (no measured data ships)
  run_sequential_stress(gens, load, weather, stress, years, storages=, ...)         run_sequential_variable's chronology with it, on the GPU
  run_analytical_stress(gens, load, weather, stress, resource_scale=)               the exact no-storage counterpart of one-year all-UP chains
  stress_report(independent, stressed)                                              the indices without and with the stress side by side (text)
"""
from __future__ import annotations

import math
import time
from dataclasses import dataclass, field

import numpy as np

from . import _abi, hl1, hl1_storage, hl1_variable

_MAX_UNITS = 128


@dataclass
class OutageStress:
    """A stress library: fail_mult[n_weather, n_classes, H] is the multiplier on the failure rate of the units of every outage class in
    every hour of every weather year (finite, >= 0; at most 8 classes), unit_class[n_units] the class of every unit of the fleet
    (-1: the unit fails at its constant rate), names optionally one name per class."""
    fail_mult: np.ndarray
    unit_class: np.ndarray
    names: tuple = ()

    def __post_init__(self):
        m = np.ascontiguousarray(self.fail_mult, dtype=np.float64)
        if m.ndim != 3:
            raise ValueError(f"OutageStress: fail_mult must be [n_weather, n_classes, hours], not {m.ndim}-dimensional")
        self.fail_mult = m
        cls = np.asarray(self.unit_class)
        if cls.ndim != 1 or not np.issubdtype(cls.dtype, np.integer):
            raise ValueError("OutageStress: unit_class must be a one-dimensional array of integers")
        self.unit_class = np.ascontiguousarray(cls, dtype=np.int32)
        self.names = tuple(self.names)

    @property
    def n_weather(self) -> int:
        return self.fail_mult.shape[0]

    @property
    def n_classes(self) -> int:
        return self.fail_mult.shape[1]

    @property
    def hours(self) -> int:
        return self.fail_mult.shape[2]


@dataclass
class StressReliabilityResult(hl1_variable.VariableReliabilityResult):
    """run_sequential_stress's result: run_sequential_variable's fields, plus the class of every unit and, per class, the mean multiplier
    over the drawn weather years."""
    unit_class: np.ndarray = field(default_factory=lambda: np.zeros(0, dtype=np.int32))
    mean_multiplier: np.ndarray = field(default_factory=lambda: np.zeros(0))


@dataclass
class AnalyticalStressResult(hl1.ReliabilityResult):
    """run_analytical_stress's result: LOLE and EUE of the first year of a chain started all UP, and the loss probability of every hour
    (the mean over the weather years)."""
    hourly_loss_probability: np.ndarray = field(default_factory=lambda: np.zeros(0))


def _stress(who: str, stress, w: hl1_variable.WeatherYears, n_units: int) -> OutageStress:
    """The checks of the library that need no device (relmc_hl1_stress_load's and relmc_hl1_stress_seq's own)."""
    s = stress if isinstance(stress, OutageStress) else OutageStress(*stress)
    if not 1 <= s.n_weather <= _abi.HL1_VAR_MAX_WEATHER:
        raise ValueError(f"{who}: n_weather {s.n_weather} not in 1..{_abi.HL1_VAR_MAX_WEATHER}")
    if not 1 <= s.n_classes <= _abi.HL1_STRESS_MAX_CLASSES:
        raise ValueError(f"{who}: n_classes {s.n_classes} not in 1..{_abi.HL1_STRESS_MAX_CLASSES}")
    if s.hours < 1:
        raise ValueError(f"{who}: the stress library has no hours")
    if s.n_weather * s.n_classes * (s.hours + 1) >= 1 << 31:
        raise ValueError(f"{who}: n_weather * n_classes * (hours + 1) is 2^31 or more")
    bad = np.argwhere(~(np.isfinite(s.fail_mult) & (s.fail_mult >= 0.0)))
    if bad.size:
        y, c, h = (int(v) for v in bad[0])
        raise ValueError(f"{who}: multiplier of weather year {y}, class {c}, hour {h} is "
                         + ("negative" if np.isfinite(s.fail_mult[y, c, h]) else "not finite"))
    if not 1 <= s.unit_class.size <= _MAX_UNITS:
        raise ValueError(f"{who}: n_units {s.unit_class.size} not in 1..{_MAX_UNITS}")
    bad = np.flatnonzero((s.unit_class < -1) | (s.unit_class >= s.n_classes))
    if bad.size:
        k = int(bad[0])
        raise ValueError(f"{who}: class {int(s.unit_class[k])} of unit {k} not in -1..{s.n_classes - 1}")
    if s.names and len(s.names) != s.n_classes:
        raise ValueError(f"{who}: {len(s.names)} names for {s.n_classes} classes")
    if s.unit_class.size != n_units:
        raise ValueError(f"{who}: the stress library has {s.unit_class.size} units, the fleet {n_units}")
    if s.n_weather != w.n_weather:
        raise ValueError(f"{who}: the stress library has {s.n_weather} weather years, the weather library {w.n_weather}")
    if s.hours != w.hours:
        raise ValueError(f"{who}: the stress library has {s.hours} hours, the weather library {w.hours}")
    return s


def _stress_load(eng, s: OutageStress) -> None:
    """relmc_hl1_stress_load, unless this library is already on the device."""
    key = (s.fail_mult.shape, s.fail_mult.tobytes(), s.unit_class.tobytes())
    if getattr(eng, "_hl1_stress_loaded", None) != key:
        eng._hl1_stress_loaded = None
        eng._check(eng.L.relmc_hl1_stress_load(eng._h, s.n_weather, s.n_classes, s.hours, s.fail_mult.ctypes.data_as(_abi.c_double_p),
                                               s.unit_class.size, s.unit_class.ctypes.data_as(_abi.c_int32_p)), "relmc_hl1_stress_load")
        eng._hl1_stress_loaded = key


def run_sequential_stress(gens, load: hl1.LoadModel, weather, stress, years: int, *, storages=(), resource_scale=None, scale: float = 1.0,
                          shift: float = 0.0, pick: str = "random", seed: int = 1, chains: int = 1, start: str = "all_up",
                          engine=None) -> StressReliabilityResult:
    """run_sequential_variable's chronology (same arguments, same weather years under the same seed) in which a UP unit of outage class
    c fails with the hazard stress.fail_mult[w, c, h] / mttf in hour h of a chain year that drew the weather year w.  A unit of class -1
    has exactly the history it has in run_sequential_variable; with every unit in class -1 the per-year arrays are that function's bit
    for bit.  start="stationary" draws the start states with the constant-rate probabilities mttr / (mttf + mttr): under a varying
    multiplier the process is not stationary."""
    from . import api
    who = "run_sequential_stress"
    years, chains = hl1._seq_shape(who, years, chains, start)
    w = hl1_variable._weather(who, weather, int(np.asarray(load.hourly_load).size))
    s = _stress(who, stress, w, len(gens))
    scale, shift = hl1_storage._level(who, scale, shift)
    rs = hl1_variable._resource_scale(who, resource_scale, w.n_resources)
    if pick not in hl1_variable._PICK:
        raise ValueError(f"{who}: pick must be one of {sorted(hl1_variable._PICK)}, not {pick!r}")
    st = hl1_storage._storages(who, storages)
    eng = engine or api.default_engine()
    t0 = time.time()
    hl1._seq_model_load(eng, gens, load)
    hl1_variable._weather_load(eng, w)
    _stress_load(eng, s)
    r = hl1_variable._run_weather_track(eng, "relmc_hl1_stress_seq", StressReliabilityResult, "Sequential MC + stress" + (" + storage" if st else ""), t0, w,
                                        years, chains, start, seed, rs, scale, shift, pick, st, unit_class=s.unit_class.copy())
    r.mean_multiplier = s.fail_mult.mean(axis=2)[r.year_weather].mean(axis=0)
    return r


def _hourly_copt(cap, qdown, net, step_size: float) -> tuple:
    """cap[K], qdown[K, n] (P(unit k DOWN) in each of n hours), net[n] -> (P(available capacity < net), E[max(net - available, 0)]) per hour:
    hl1.run_analytical's outage table with its capacity rounding (hl1.convolve_unit), one table per hour, vectorised over the hours."""
    n = net.size
    size = int(sum(math.ceil(c / step_size) + 1 for c in cap)) + 1
    P = np.zeros((n, size))
    P[:, 0] = 1.0
    top = 0                                                        # the highest state that can hold probability
    for k, c in enumerate(cap):
        q = qdown[k][:, None]
        lower = int(math.floor(c / step_size))
        alpha = (c - lower * step_size) / step_size
        new = P * (1.0 - q)
        if abs(c - lower * step_size) < 1e-5:
            new[:, lower:lower + top + 1] += P[:, :top + 1] * q
            top += lower
        else:
            new[:, lower:lower + top + 1] += P[:, :top + 1] * (q * (1.0 - alpha))
            new[:, lower + 1:lower + top + 2] += P[:, :top + 1] * (q * alpha)
            top += lower + 1
        P = new
    outage = np.arange(size) * step_size
    reserve = float(np.sum(cap)) - net                             # a loss: outage > reserve
    short = outage[None, :] > reserve[:, None]
    return (P * short).sum(axis=1), (P * short * (outage[None, :] - reserve[:, None])).sum(axis=1)


def run_analytical_stress(gens, load: hl1.LoadModel, weather, stress, resource_scale=None, step_size: float = 1.0) -> AnalyticalStressResult:
    """The exact no-storage counterpart of run_sequential_stress for one-year chains started all UP (years == chains,
    start="all_up"), the weather years taken with equal weight.  Within an hour a unit's rates are constant, so with
    lam = fail_mult / mttf (1 / mttf for class -1) and mu = 1 / mttr the probability that it is DOWN at step n is
    p_n = p_inf + (p_(n-1) - p_inf) * exp(-(lam + mu)), p_inf = lam / (lam + mu), p_0 = 0.  LOLE and EUE are the sums over the hours of an
    hourly outage table (hl1.run_analytical's, with its capacity step) against the net load L_w - v_w, v_w the sum of
    resource_scale[r] * output; the result also holds the loss probability of every hour."""
    who = "run_analytical_stress"
    t0 = time.time()
    w = hl1_variable._weather(who, weather, int(np.asarray(load.hourly_load).size))
    s = _stress(who, stress, w, len(gens))
    rs = np.asarray(hl1_variable._resource_scale(who, resource_scale, w.n_resources))
    if not (math.isfinite(step_size) and step_size > 0.0):
        raise ValueError(f"{who}: step_size must be positive")
    H, K = w.hours, len(gens)
    cap = [float(g.capacity) for g in gens]
    mu = np.array([1.0 / g.mttr for g in gens])
    lole = eue = 0.0
    hourly = np.zeros(H)
    for y in range(w.n_weather):
        base = w.load_mw[y] if w.load_mw is not None else np.asarray(load.hourly_load, dtype=np.float64)
        v = (rs[:, None] * w.output_mw[y]).sum(axis=0) if w.n_resources else 0.0
        net = np.asarray(base - v, dtype=np.float64)
        mult = np.where(s.unit_class[:, None] >= 0, s.fail_mult[y][np.maximum(s.unit_class, 0)], 1.0)      # [K, H]
        lam = mult / np.array([g.mttf for g in gens])[:, None]
        pinf, decay = lam / (lam + mu[:, None]), np.exp(-(lam + mu[:, None]))
        q = np.zeros((K, H))
        p = np.zeros(K)
        for n in range(H):                                         # the recursion, all units at once
            p = pinf[:, n] + (p - pinf[:, n]) * decay[:, n]
            q[:, n] = p
        for b in range(0, H, 256):                                 # the hourly tables, 256 hours at a time
            pl, pe = _hourly_copt(cap, q[:, b:b + 256], net[b:b + 256], step_size)
            hourly[b:b + 256] += pl
            lole += float(pl.sum())
            eue += float(pe.sum())
    nwy = w.n_weather
    return AnalyticalStressResult("Analytical + outage stress", lole / nwy, eue / nwy, time.time() - t0, hourly_loss_probability=hourly / nwy)


def synthetic_stress(weather, load: hl1.LoadModel, gens, *, sensitivity=(6.0, 2.0), threshold: float = 0.85, large_mw: float = None,
                     names=("large thermal", "small thermal")) -> OutageStress:
    """An ILLUSTRATIVE stress library (as hl1_variable.synthetic_weather is illustrative: no measured data ships, and nothing here is
    fitted to any fleet).  The multipliers rise with the weather year's own load curve (`load` when the library has none): with x the
    hour's load over the library's peak load, class c gets 1 + sensitivity[c] * (max(0, x - threshold) / (1 - threshold))^2, and every
    class is then divided by its mean over the whole library.  Every class therefore has mean 1: against a run without stress, a
    run with it isolates the correlation of outages with the load.  Units of at least large_mw (default: the median capacity) are
    class 0, the others class 1; with one sensitivity every unit is class 0."""
    who = "synthetic_stress"
    w = hl1_variable._weather(who, weather, int(np.asarray(load.hourly_load).size))
    sens = tuple(float(v) for v in sensitivity)
    if not 1 <= len(sens) <= 2 or not all(math.isfinite(v) and v >= 0.0 for v in sens):
        raise ValueError(f"{who}: sensitivity must be one or two finite values that are not negative")
    if not 0.0 <= threshold < 1.0:
        raise ValueError(f"{who}: threshold must be in [0, 1)")
    if not gens:
        raise ValueError(f"{who}: no units")
    curves = w.load_mw if w.load_mw is not None else np.tile(np.asarray(load.hourly_load, dtype=np.float64), (w.n_weather, 1))
    peak = float(curves.max())
    if not peak > 0.0:
        raise ValueError(f"{who}: the load is not positive")
    x = np.maximum(curves / peak - threshold, 0.0) / (1.0 - threshold)
    mult = np.stack([1.0 + b * x * x for b in sens], axis=1)       # [n_weather, n_classes, H]
    mult /= mult.mean(axis=(0, 2), keepdims=True)
    caps = np.array([g.capacity for g in gens], dtype=np.float64)
    cut = float(np.median(caps)) if large_mw is None else float(large_mw)
    cls = np.where(caps >= cut, 0, 1).astype(np.int32) if len(sens) == 2 else np.zeros(caps.size, dtype=np.int32)
    return OutageStress(mult, cls, tuple(names)[:len(sens)])


def stress_report(independent: hl1.SequentialReliabilityResult, stressed: StressReliabilityResult) -> str:
    """LOLE, EUE and LOLF with independent outages and with the stress side by side, and what the stress was, in variable_report's style."""
    rule = "=" * 42
    lines = [rule, "    OUTAGE STRESS SUMMARY", rule,
             "%-36s | %-10s | %-10s | %-12s" % ("Method", "LOLE(h/yr)", "EUE(MWh)", "LOLF(occ/yr)"), "-" * 78]
    lines += ["%-36s | %-10.4f | %-10.2f | %-12.4f" % (r.method, r.lole_hours_yr, r.eue_mwh_yr, r.lolf_occ_yr) for r in (independent, stressed)]
    lines.append("-" * 78)
    s = stressed
    n = int((s.unit_class >= 0).sum())
    nwy = np.unique(s.year_weather).size
    lines.append("%d of %d unit%s in %d outage class%s over %d weather year%s drawn (%s); mean multiplier per class: %s"
                 % (n, s.unit_class.size, "" if s.unit_class.size == 1 else "s", s.mean_multiplier.size, "" if s.mean_multiplier.size == 1 else "es",
                    nwy, "" if nwy == 1 else "s", s.pick, ", ".join("%.3f" % v for v in s.mean_multiplier)))
    if independent.lole_hours_yr > 0 and independent.eue_mwh_yr > 0:
        lines.append("LOLE x %.3f, EUE x %.3f against independent outages"
                     % (s.lole_hours_yr / independent.lole_hours_yr, s.eue_mwh_yr / independent.eue_mwh_yr))
    return "\n".join(lines) + "\n"
