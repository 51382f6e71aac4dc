"""Weather-year wind and solar resources on the HL1 sequential chronology, with storage — an extension beyond the reference, whose
generation is all dispatchable (a unit is UP or DOWN and gives its full capacity when UP).

The output of wind and solar is an hourly profile that differs from weather year to weather year and is correlated with the load of the
same weather year.  A WeatherYears library holds such years; every chain year of a run draws one of them, the fleet fails and repairs
as in run_sequential_mc, and the storages of hl1_storage.py charge from the surplus that now includes the resources' output
(relmc_hl1_var_load, relmc_hl1_var_seq; the rules are written out in include/relmc.h).

  WeatherYears(output_mw[n_weather, n_resources, H], load_mw=None, names=())   the library; load_mw[n_weather, H]: each year's own load curve
  synthetic_weather(n_weather, hours, solar_mw=, wind_mw=, seed=)             an illustrative solar + wind library (no measured data ships)
  run_sequential_variable(gens, load, weather, years, storages=, ...)        run_sequential_mc's chronology with the resources, on the GPU
  run_analytical_variable(gens, weather, load, resource_scale=)              the exact no-storage counterpart (mean over the weather years)
  resource_elcc(gens, load, weather, resources, years)                       what resources are worth in load (hl1.CarryingCapabilityResult)
  variable_report(base, with_resources)                                      the indices without and with the resources side by side (text)
"""
from __future__ import annotations

import ctypes as C
import math
import time
from dataclasses import dataclass, field

import numpy as np

from . import _abi, hl1, hl1_storage
from .hl1_areas import _first_crossing, _interpolate_pair

_PICK = {"random": _abi.HL1_VAR_PICK_RANDOM, "cycle": _abi.HL1_VAR_PICK_CYCLE}


@dataclass
class WeatherYears:
    """A library of weather years: output_mw[n_weather, n_resources, H] is the hourly output in MW of every resource in every weather
    year (finite, >= 0; n_resources may be 0), load_mw[n_weather, H] optionally the load curve of each weather year (without it every
    year sees the load given to the run), names optionally one name per resource."""
    output_mw: np.ndarray
    load_mw: np.ndarray = None
    names: tuple = ()

    def __post_init__(self):
        out = np.ascontiguousarray(self.output_mw, dtype=np.float64)
        if out.ndim != 3:
            raise ValueError(f"WeatherYears: output_mw must be [n_weather, n_resources, hours], not {out.ndim}-dimensional")
        self.output_mw = out
        if self.load_mw is not None:
            self.load_mw = np.ascontiguousarray(self.load_mw, dtype=np.float64)
        self.names = tuple(self.names)

    @property
    def n_weather(self) -> int:
        return self.output_mw.shape[0]

    @property
    def n_resources(self) -> int:
        return self.output_mw.shape[1]

    @property
    def hours(self) -> int:
        return self.output_mw.shape[2]


@dataclass
class VariableReliabilityResult(hl1_storage.StorageReliabilityResult):
    """run_sequential_variable's result: run_sequential_storage's fields, plus the weather year of every simulated year (the per-year
    arrays' order: chain-major) and the mean, over the drawn weather years, of the scaled resource energy."""
    year_weather: np.ndarray = field(default_factory=lambda: np.zeros(0, dtype=np.int32))
    offered_mwh_yr: float = 0.0
    resource_scale: tuple = ()
    pick: str = "random"


def _weather(who: str, weather, hours: int) -> WeatherYears:
    """The checks of the library that need no device (relmc_hl1_var_load's own, in its order)."""
    w = weather if isinstance(weather, WeatherYears) else WeatherYears(*weather)
    if not 1 <= w.n_weather <= _abi.HL1_VAR_MAX_WEATHER:
        raise ValueError(f"{who}: n_weather {w.n_weather} not in 1..{_abi.HL1_VAR_MAX_WEATHER}")
    if w.n_resources > _abi.HL1_VAR_MAX_RESOURCES:
        raise ValueError(f"{who}: n_resources {w.n_resources} not in 0..{_abi.HL1_VAR_MAX_RESOURCES}")
    if w.hours < 1:
        raise ValueError(f"{who}: the weather years have no hours")
    if w.n_weather * max(w.n_resources, 1) * w.hours >= 1 << 31:
        raise ValueError(f"{who}: n_weather * max(n_resources, 1) * hours is 2^31 or more")
    bad = np.argwhere(~(np.isfinite(w.output_mw) & (w.output_mw >= 0.0)))
    if bad.size:
        y, r, h = (int(v) for v in bad[0])
        raise ValueError(f"{who}: output of weather year {y}, resource {r}, hour {h} is "
                         + ("negative" if np.isfinite(w.output_mw[y, r, h]) else "not finite"))
    if w.load_mw is not None:
        if w.load_mw.shape != (w.n_weather, w.hours):
            raise ValueError(f"{who}: load_mw must be [{w.n_weather}, {w.hours}], not {list(w.load_mw.shape)}")
        bad = np.argwhere(~np.isfinite(w.load_mw))
        if bad.size:
            raise ValueError(f"{who}: load of weather year {int(bad[0][0])}, hour {int(bad[0][1])} not finite")
    if w.hours != hours:
        raise ValueError(f"{who}: the load curve has {hours} hours, the weather years {w.hours}")
    return w


def _resource_scale(who: str, resource_scale, n_resources: int) -> tuple:
    rs = (1.0,) * n_resources if resource_scale is None else tuple(float(v) for v in resource_scale)
    if len(rs) != n_resources:
        raise ValueError(f"{who}: {len(rs)} resource scales for {n_resources} resources")
    for r, v in enumerate(rs):
        if not math.isfinite(v):
            raise ValueError(f"{who}: resource_scale {r} not finite")
        if v < 0.0:
            raise ValueError(f"{who}: resource_scale {r} is negative")
    return rs


def _weather_load(eng, w: WeatherYears) -> None:
    """relmc_hl1_var_load, unless this library is already on the device."""
    key = (w.output_mw.shape, w.output_mw.tobytes(), None if w.load_mw is None else w.load_mw.tobytes())
    if getattr(eng, "_hl1_var_loaded", None) != key:
        eng._hl1_var_loaded = None
        eng._check(eng.L.relmc_hl1_var_load(eng._h, w.n_weather, w.n_resources, w.hours,
                                            w.output_mw.ctypes.data_as(_abi.c_double_p) if w.n_resources else None,
                                            None if w.load_mw is None else w.load_mw.ctypes.data_as(_abi.c_double_p)), "relmc_hl1_var_load")
        eng._hl1_var_loaded = key


def _run_weather_track(eng, entry: str, result, method: str, t0: float, w: WeatherYears, years: int, chains: int, start: str, seed: int,
                       rs: tuple, scale: float, shift: float, pick: str, st: tuple, **more):
    """The call of `entry` (relmc_hl1_var_seq, or relmc_hl1_stress_seq, which has its signature) on the models already loaded, and its
    outputs as a `result` (VariableReliabilityResult or a subclass; `more`: the subclass's own fields).  The arguments are checked."""
    opts = _abi.Hl1VarOpts()
    for r, v in enumerate(rs):
        opts.resource_scale[r] = v
    opts.scale, opts.shift, opts.pick, opts.reserved = scale, shift, _PICK[pick], 0
    arr = (_abi.Hl1Storage * max(len(st), 1))(*[_abi.Hl1Storage(float(s.charge_mw), float(s.discharge_mw), float(s.energy_mwh),
                                                                 float(s.eta_charge), float(s.eta_discharge), s.soc0) for s in st])
    acc = _abi.Hl1StorageAcc()
    yr, sy, wy = np.zeros((years, 3)), np.zeros((years, 3)), np.zeros(years, dtype=np.int32)
    eng._check(getattr(eng.L, entry)(eng._h, int(seed), 0, chains, years // chains, hl1._SEQ_START[start], C.byref(opts), len(st),
                                     arr if st else None, C.byref(acc), yr.ctypes.data_as(C.POINTER(_abi.Hl1SeqYear)),
                                     sy.ctypes.data_as(C.POINTER(_abi.Hl1StorageYear)), wy.ctypes.data_as(_abi.c_int32_p)), entry)
    k = np.arange(10, years + 1, 10)
    history = np.cumsum(yr[:, 0])[k - 1] / k if k.size else np.zeros(0)
    lole, eue, lolf = acc.sum_lole / years, acc.sum_eue / years, acc.sum_lolf / years
    energy = (w.output_mw.sum(axis=2) * np.asarray(rs)[None, :]).sum(axis=1) if w.n_resources else np.zeros(w.n_weather)
    return result(method, lole, eue, time.time() - t0, history,
                  lolf_occ_yr=lolf, lold_hours=lole / lolf if lolf > 0 else float("nan"),
                  year_lole=yr[:, 0].copy(), year_eue=yr[:, 1].copy(), year_lolf=yr[:, 2].copy(),
                  served_hours_yr=acc.sum_served / years, discharged_mwh_yr=acc.sum_discharged / years,
                  charged_mwh_yr=acc.sum_charged / years, year_served=sy[:, 0].copy(), year_discharged=sy[:, 1].copy(),
                  year_charged=sy[:, 2].copy(), storages=st, scale=scale, shift=shift,
                  year_weather=wy, offered_mwh_yr=float(energy[wy].mean()), resource_scale=rs, pick=pick, **more)


def run_sequential_variable(gens, load: hl1.LoadModel, weather, years: int, *, storages=(), resource_scale=None, scale: float = 1.0,
                            shift: float = 0.0, pick: str = "random", seed: int = 1, chains: int = 1, start: str = "all_up",
                            engine=None) -> VariableReliabilityResult:
    """run_sequential_mc's chronology (same arguments, same chains under the same seed) with the resources of `weather` (a WeatherYears)
    and the storages `storages` (hl1_storage.Storage objects, at most 8).  Every chain year draws a weather year: pick="random" by a
    counter-based draw of its own, pick="cycle" in turn, (chain * years_per_chain + year) mod n_weather.  The step's capacity is the
    fleet's plus resource_scale[r] * output (None: every resource at 1.0; 0 withholds a resource), its load scale * base + shift with
    base the weather year's own load curve when the library has them, else `load`.  Without resources and storages, and without load
    curves in the library, the per-year arrays are run_sequential_mc's bit for bit."""
    from . import api
    who = "run_sequential_variable"
    years, chains = hl1._seq_shape(who, years, chains, start)
    w = _weather(who, weather, int(np.asarray(load.hourly_load).size))
    scale, shift = hl1_storage._level(who, scale, shift)
    rs = _resource_scale(who, resource_scale, w.n_resources)
    if pick not in _PICK:
        raise ValueError(f"{who}: pick must be one of {sorted(_PICK)}, not {pick!r}")
    st = hl1_storage._storages(who, storages)
    eng = engine or api.default_engine()
    t0 = time.time()
    hl1._seq_model_load(eng, gens, load)
    _weather_load(eng, w)
    method = "Sequential MC + resources" + (" + storage" if st else "") if any(v > 0.0 for v in rs) else "Sequential MC" + (" + storage" if st else "")
    return _run_weather_track(eng, "relmc_hl1_var_seq", VariableReliabilityResult, method, t0, w, years, chains, start, seed, rs, scale, shift, pick, st)


def run_analytical_variable(gens, weather, load: hl1.LoadModel, resource_scale=None, step_size: float = 1.0) -> hl1.ReliabilityResult:
    """The exact no-storage counterpart of run_sequential_variable in the stationary state: the mean, over the weather years taken with
    equal weight, of hl1.run_analytical against the net load max(L_w - v_w, 0), with L_w the weather year's load curve (`load` when the
    library has none) and v_w the sum of resource_scale[r] * output."""
    who = "run_analytical_variable"
    t0 = time.time()
    w = _weather(who, weather, int(np.asarray(load.hourly_load).size))
    rs = np.asarray(_resource_scale(who, resource_scale, w.n_resources))
    lole = eue = 0.0
    for y in range(w.n_weather):
        base = w.load_mw[y] if w.load_mw is not None else np.asarray(load.hourly_load, dtype=np.float64)
        v = (rs[:, None] * w.output_mw[y]).sum(axis=0) if w.n_resources else 0.0
        r = hl1.run_analytical(gens, hl1.LoadModel(np.maximum(base - v, 0.0)), step_size=step_size)
        lole += r.lole_hours_yr
        eue += r.eue_mwh_yr
    return hl1.ReliabilityResult("Analytical + resources", lole / w.n_weather, eue / w.n_weather, time.time() - t0)


def variable_report(base: hl1.SequentialReliabilityResult, with_resources: VariableReliabilityResult) -> str:
    """LOLE, EUE and LOLF without and with the resources side by side, the energy they offer and what the storages cycled per year, in
    storage_report's style."""
    rule = "=" * 42
    lines = [rule, "    VARIABLE RESOURCE SUMMARY", rule,
             "%-36s | %-10s | %-10s | %-12s" % ("Method", "LOLE(h/yr)", "EUE(MWh)", "LOLF(occ/yr)"), "-" * 78]
    lines += ["%-36s | %-10.4f | %-10.2f | %-12.4f" % (r.method, r.lole_hours_yr, r.eue_mwh_yr, r.lolf_occ_yr) for r in (base, with_resources)]
    lines.append("-" * 78)
    s = with_resources
    n = sum(1 for v in s.resource_scale if v > 0.0)
    lines.append("%d resource%s over %d weather year%s drawn (%s): %.2f MWh/yr offered"
                 % (n, "" if n == 1 else "s", np.unique(s.year_weather).size, "" if np.unique(s.year_weather).size == 1 else "s", s.pick,
                    s.offered_mwh_yr))
    if s.storages:
        lines.append("%d storage%s: %.4f short hours/yr served in full, %.2f MWh/yr delivered, %.2f MWh/yr of surplus taken"
                     % (len(s.storages), "" if len(s.storages) == 1 else "s", s.served_hours_yr, s.discharged_mwh_yr, s.charged_mwh_yr))
    return "\n".join(lines) + "\n"


def resource_elcc(gens, load: hl1.LoadModel, weather, resources, years: int, *, storages=(), resource_scale=None, pick: str = "random",
                  metric: str = "lole", bracket=None, rounds: int = 3, seed: int = 1, chains: int = 1, start: str = "all_up",
                  engine=None) -> hl1.CarryingCapabilityResult:
    """What the resources `resources` (0-based indices into the library's resources) are worth in load: the load shift in MW after which
    the system with them is as risky as the system with their scale 0 at the unshifted load, every other resource and the storages
    being there in both.  The target is run_sequential_variable's metric with the chosen scales at 0, under the same seed, chains,
    start and pick, so both sides see the same fleet history and the same weather years.  Each round evaluates 8 equally spaced shifts
    and keeps the first adjacent pair that brackets the target; the last pair is interpolated linearly.  The chosen resources deliver
    at most max over weather year and hour of their summed scaled output, so the default bracket (0, that maximum) holds the root.
    Without storages the sampled metric is monotone in the shift (the capacity of every step is the same and its load rises); with
    storages no monotonicity is claimed, and ValueError is raised when no pair brackets.  The standard error comes from the per-year
    paired differences between the interpolated pair and the target, over the slope."""
    who = "resource_elcc"
    years, chains = hl1._seq_shape(who, years, chains, start)
    w = _weather(who, weather, int(np.asarray(load.hourly_load).size))
    rs = _resource_scale(who, resource_scale, w.n_resources)
    if pick not in _PICK:
        raise ValueError(f"{who}: pick must be one of {sorted(_PICK)}, not {pick!r}")
    st = hl1_storage._storages(who, storages)
    chosen = sorted({int(r) for r in resources})
    if not chosen:
        raise ValueError(f"{who}: no resource given")
    if chosen[0] < 0 or chosen[-1] >= w.n_resources:
        raise ValueError(f"{who}: resources must be indices in 0..{w.n_resources - 1}, not {chosen}")
    top = float((np.asarray([rs[r] for r in chosen])[None, :, None] * w.output_mw[:, chosen, :]).sum(axis=1).max())
    if bracket is None and not top > 0.0:
        raise ValueError(f"{who}: the chosen resources have no output")
    lo, hi, rounds = hl1._search_args(who, metric, "shift", (0.0, top) if bracket is None else bracket, rounds)
    t0 = time.time()
    kw = dict(storages=st, pick=pick, seed=seed, chains=chains, start=start, engine=engine)
    per_year, attr = "year_" + metric, hl1._SWEEP_METRIC[metric]
    without = tuple(0.0 if r in chosen else v for r, v in enumerate(rs))
    base = run_sequential_variable(gens, load, w, years, resource_scale=without, **kw)
    target, target_year = float(getattr(base, attr)), getattr(base, per_year)
    for _ in range(rounds):
        x = np.linspace(lo, hi, 8)
        runs = [run_sequential_variable(gens, load, w, years, resource_scale=rs, shift=float(v), **kw) for v in x]
        m = np.array([getattr(r, attr) for r in runs])
        i = _first_crossing(who, m, target)
        lo, hi = float(x[i]), float(x[i + 1])
    value, t, slope = _interpolate_pair(x, m, i, target)
    se_d = float(hl1._se((1.0 - t) * getattr(runs[i], per_year) + t * getattr(runs[i + 1], per_year) - target_year))
    return hl1.CarryingCapabilityResult("Sequential MC + resources", metric, "shift", value, se_d / abs(slope) if slope != 0 else float("inf"),
                                        (lo, hi), (float(m[i]), float(m[i + 1])), target, years, rounds, time.time() - t0, [target_year.copy()])


def synthetic_weather(n_weather: int, hours: int = 8736, solar_mw: float = 300.0, wind_mw: float = 300.0, seed: int = 2026,
                      load: hl1.LoadModel = None) -> WeatherYears:
    """An ILLUSTRATIVE library of n_weather weather years with two resources, ("solar", "wind"), from a deterministic numpy generator
    (as hl1_multistate.derated_rts24() is illustrative: no measured data ships, and nothing here is fitted to any site).
      solar  a clear-sky shape, max(0, sin) of the hour of the day between 06:00 and 18:00 times a seasonal factor 0.6 + 0.4 * cos around
             the year's middle, times a daily cloud factor drawn uniformly in [0.25, 1]; zero at night
      wind   an AR(1) series x_h = 0.97 x_(h-1) + sqrt(1 - 0.97^2) e_h with standard normal e, mapped to [0, 1] by the logistic function
             of 1.5 x - 0.5 (a capacity factor near 0.4)
    Both stay within [0, nameplate].  With `load` given, every weather year also gets a load curve: `load` times (1 + 0.03 z_d) per day,
    z_d standard normal clipped to [-2, 2] (hot and cold spells), so that the library's load differs from year to year as its weather does."""
    n_weather, hours = int(n_weather), int(hours)
    if n_weather < 1 or hours < 1:
        raise ValueError("synthetic_weather: n_weather and hours must be positive")
    if not (math.isfinite(solar_mw) and math.isfinite(wind_mw) and solar_mw >= 0.0 and wind_mw >= 0.0):
        raise ValueError("synthetic_weather: solar_mw and wind_mw must be finite and not negative")
    rng = np.random.default_rng(int(seed))
    h = np.arange(hours)
    hod, day = h % 24, h // 24
    ndays = int(day[-1]) + 1
    clear = np.where((hod > 6) & (hod < 18), np.sin(np.pi * (hod - 6.0) / 12.0), 0.0) * (0.6 + 0.4 * np.cos(2.0 * np.pi * (h / hours - 0.5)))
    out = np.zeros((n_weather, 2, hours))
    curves = None if load is None else np.zeros((n_weather, hours))
    a = 0.97
    for y in range(n_weather):
        cloud = rng.uniform(0.25, 1.0, ndays)
        out[y, 0] = np.clip(solar_mw * clear * cloud[day], 0.0, solar_mw)
        e = rng.standard_normal(hours) * math.sqrt(1.0 - a * a)
        x = np.empty(hours)
        prev = rng.standard_normal()
        for i in range(hours):
            prev = a * prev + e[i]
            x[i] = prev
        out[y, 1] = np.clip(wind_mw / (1.0 + np.exp(-(1.5 * x - 0.5))), 0.0, wind_mw)
        if curves is not None:
            z = np.clip(rng.standard_normal(ndays), -2.0, 2.0)
            curves[y] = np.asarray(load.hourly_load, dtype=np.float64) * (1.0 + 0.03 * z[day])
    return WeatherYears(out, curves, ("solar", "wind"))
