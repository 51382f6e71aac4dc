"""Weather-year resources and storages in the areas of the HL1 multi-area chronology — an extension beyond the reference, whose areas
hold dispatchable two-state units against one fixed load curve each.

What wind, solar and a battery in area B are worth to B and to its neighbours across a limited tie exists only on the multi-area
chronology.  An AreaWeatherYears library holds the hourly output of up to 8 resources, each placed in an area, in every weather year,
and optionally a load curve of every area; every chain year of a run draws one weather year, the units and ties fail and repair as in
hl1_areas.run_fast_sequential_simulation, the areas help each other over the ties FIRST, and the storages of an area then discharge into
what is left of its deficit or charge from what is left of its surplus (relmc_hl1_area_var_load, relmc_hl1_area_var; the rules are
written out in include/relmc.h).  Energy-limited resources are used after the ties: a storage neither exports nor charges from imports.

  AreaWeatherYears(output_mw[n_weather, n_resources, H], resource_area, load_mw=None, names=())   the library; areas 1-based, as TieLine
  AreaStorage(area, storage)                                      an hl1_storage.Storage in the 1-based area `area`
  run_area_variable(sys, policy, weather, n_years, storages=, ...)    the multi-area chronology with the resources and storages, on the GPU
  area_variable_report(base, result)                              the rows without and with the resources and storages side by side (text)
  area_resource_elcc(sys, weather, area, n_years, resources=, storages=, ...)   what they are worth in load of an area
  synthetic_area_weather(sys, n_weather, ...)                     an illustrative library built from hl1_variable.synthetic_weather
"""
from __future__ import annotations

import ctypes as C
import math
import time
from dataclasses import dataclass, field

import numpy as np

from . import _abi, hl1, hl1_areas, hl1_storage, hl1_variable
from .hl1_areas import MultiAreaResult, SupportPolicy, System, _first_crossing, _interpolate_pair

_PICK = hl1_variable._PICK


@dataclass
class AreaWeatherYears:
    """A library of weather years for a multi-area system: output_mw[n_weather, n_resources, H] is the hourly output in MW of every
    resource in every weather year (finite, >= 0; n_resources may be 0), resource_area[r] the 1-based area of resource r (as TieLine),
    load_mw[n_weather, n_areas, H] optionally the load curve of every area in every weather year (without it every year sees the areas'
    own curves), names optionally one name per resource."""
    output_mw: np.ndarray
    resource_area: tuple
    load_mw: np.ndarray = None
    names: tuple = ()

    def __post_init__(self):
        out = np.ascontiguousarray(self.output_mw, dtype=np.float64)
        if out.ndim != 3:
            raise ValueError(f"AreaWeatherYears: output_mw must be [n_weather, n_resources, hours], not {out.ndim}-dimensional")
        self.output_mw = out
        self.resource_area = tuple(int(a) for a in self.resource_area)
        if len(self.resource_area) != out.shape[1]:
            raise ValueError(f"AreaWeatherYears: {len(self.resource_area)} resource areas for {out.shape[1]} resources")
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
class AreaStorage:
    """The storage `storage` (an hl1_storage.Storage) in area `area`, 1-based as TieLine (converted at the ABI).  The storages of one
    area act in the order in which they are given."""
    area: int
    storage: hl1_storage.Storage


@dataclass
class AreaVariableResult(MultiAreaResult):
    """run_area_variable's result: MultiAreaResult's fields (results, lolf, lold, the system row, year_indices[year, row, 3]) after the
    storages, plus per row (areas, then the system) the short hours served in full, the MWh delivered and the MWh of surplus taken per
    year, their per-year arrays year_storage[year, row, (served, discharged, charged)], and the weather year of every simulated year
    (chain-major, as the per-year arrays)."""
    served_hours: np.ndarray = field(default_factory=lambda: np.zeros(0))
    discharged_mwh: np.ndarray = field(default_factory=lambda: np.zeros(0))
    charged_mwh: np.ndarray = field(default_factory=lambda: np.zeros(0))
    year_storage: np.ndarray = field(default_factory=lambda: np.zeros((0, 0, 3)))
    year_weather: np.ndarray = field(default_factory=lambda: np.zeros(0, dtype=np.int32))
    resource_scale: tuple = ()
    load_scale: tuple = ()
    load_shift: tuple = ()
    storages: tuple = ()
    pick: str = "random"


def _area_weather(who: str, weather, n_areas: int, hours: int) -> AreaWeatherYears:
    """The checks of the library that need no device (relmc_hl1_area_var_load's own, in its order)."""
    w = weather if isinstance(weather, AreaWeatherYears) else AreaWeatherYears(*weather)
    if not 1 <= w.n_weather <= _abi.HL1_VAR_MAX_WEATHER:
        raise ValueError(f"{who}: n_weather {w.n_weather} not in 1..{_abi.HL1_VAR_MAX_WEATHER}")
    if w.n_resources > _abi.HL1_VAR_MAX_RESOURCES:
        raise ValueError(f"{who}: n_resources {w.n_resources} not in 0..{_abi.HL1_VAR_MAX_RESOURCES}")
    if w.hours < 1:
        raise ValueError(f"{who}: the weather years have no hours")
    for r, a in enumerate(w.resource_area):
        if not 1 <= a <= n_areas:
            raise ValueError(f"{who}: resource {r} is in area {a}, not in 1..{n_areas} (1-based, as TieLine)")
    if w.n_weather * max(w.n_resources, n_areas, 1) * w.hours >= 1 << 31:
        raise ValueError(f"{who}: n_weather * max(n_resources, n_areas, 1) * hours is 2^31 or more")
    bad = np.argwhere(~(np.isfinite(w.output_mw) & (w.output_mw >= 0.0)))
    if bad.size:
        y, r, h = (int(v) for v in bad[0])
        raise ValueError(f"{who}: output of weather year {y}, resource {r}, hour {h} is "
                         + ("negative" if np.isfinite(w.output_mw[y, r, h]) else "not finite"))
    if w.load_mw is not None:
        if w.load_mw.shape != (w.n_weather, n_areas, w.hours):
            raise ValueError(f"{who}: load_mw must be [{w.n_weather}, {n_areas}, {w.hours}], not {list(w.load_mw.shape)}")
        bad = np.argwhere(~np.isfinite(w.load_mw))
        if bad.size:
            raise ValueError(f"{who}: load of weather year {int(bad[0][0])}, area {int(bad[0][1]) + 1}, hour {int(bad[0][2])} not finite")
    if w.hours != hours:
        raise ValueError(f"{who}: the areas' load curves have {hours} hours, the weather years {w.hours}")
    return w


def _per_area(who: str, name: str, values, n_areas: int, default: float) -> tuple:
    v = (default,) * n_areas if values is None else tuple(float(x) for x in values)
    if len(v) != n_areas:
        raise ValueError(f"{who}: {len(v)} values of {name} for {n_areas} areas")
    for a, x in enumerate(v):
        if not math.isfinite(x):
            raise ValueError(f"{who}: {name} of area {a + 1} not finite")
    return v


def _area_storages(who: str, storages, n_areas: int) -> tuple:
    st = tuple(s if isinstance(s, AreaStorage) else AreaStorage(*s) for s in storages)
    if len(st) > _abi.HL1_MAX_STORAGE:
        raise ValueError(f"{who}: {len(st)} storages; {_abi.HL1_MAX_STORAGE} at most, all areas together")
    for i, s in enumerate(st):
        if not (isinstance(s.area, (int, np.integer)) and 1 <= int(s.area) <= n_areas):
            raise ValueError(f"{who}: storage {i} is in area {s.area!r}, not in 1..{n_areas} (1-based, as TieLine)")
    hl1_storage._storages(who, [s.storage for s in st])          # the field rules, naming the storage and the field
    return st


def _library_load(eng, w: AreaWeatherYears, n_areas: int) -> None:
    """relmc_hl1_area_var_load, unless this library is already on the device."""
    key = (n_areas, w.output_mw.shape, w.output_mw.tobytes(), w.resource_area, None if w.load_mw is None else w.load_mw.tobytes())
    if getattr(eng, "_hl1_area_var_loaded", None) != key:
        eng._hl1_area_var_loaded = None
        ra = np.ascontiguousarray([a - 1 for a in w.resource_area], dtype=np.int32)
        eng._check(eng.L.relmc_hl1_area_var_load(eng._h, n_areas, w.n_weather, w.n_resources, ra.ctypes.data_as(_abi.c_int32_p) if ra.size else None,
                                                 w.hours, w.output_mw.ctypes.data_as(_abi.c_double_p) if w.n_resources else None,
                                                 None if w.load_mw is None else w.load_mw.ctypes.data_as(_abi.c_double_p)), "relmc_hl1_area_var_load")
        eng._hl1_area_var_loaded = key


def run_area_variable(sys: System, policy, weather, n_years: int, *, storages=(), resource_scale=None, load_scale=None, load_shift=None,
                      pick: str = "random", flow: str = "reference", seed: int = 1, chains: int = 1, start: str = "all_up",
                      engine=None) -> AreaVariableResult:
    """hl1_areas.run_fast_sequential_simulation's chronology (same arguments, same chains under the same seed, the tie outages of `sys`
    included) with the resources of `weather` (an AreaWeatherYears) and the storages `storages` (AreaStorage objects, at most 8 in all).
    Every chain year draws a weather year (pick as in hl1_variable.run_sequential_variable).  Area a's capacity is its UP units' plus
    resource_scale[r] * output of its resources (None: every resource at 1.0; 0 withholds one), its load load_scale[a] * base +
    load_shift[a] (per area, None: 1 / 0) with base the weather year's curve of the area when the library has them.  Under INTERCONNECTED
    the areas help each other first; then each area's storages serve what is left of its deficit, or charge from what is left of its
    surplus.  Without resources, storages and library curves the per-year indices are run_fast_sequential_simulation's bit for bit."""
    from . import api
    who = "run_area_variable"
    n_years, chains = hl1._seq_shape(who, n_years, chains, start)
    if flow not in hl1_areas._FLOW:
        raise ValueError(f"{who}: flow must be one of {sorted(hl1_areas._FLOW)}, not {flow!r}")
    if policy not in (hl1_areas.ISOLATED, hl1_areas.INTERCONNECTED):
        raise ValueError(f"{who}: policy must be ISOLATED or INTERCONNECTED, not {policy!r}")
    policy = SupportPolicy(policy)
    if pick not in _PICK:
        raise ValueError(f"{who}: pick must be one of {sorted(_PICK)}, not {pick!r}")
    units, cap, mttf, mttr, load, tf, tt, tc = hl1_areas._flatten(sys)
    kf, kr = hl1_areas._tie_outages(sys)
    n = units.size
    w = _area_weather(who, weather, n, load.shape[1])
    rs = hl1_variable._resource_scale(who, resource_scale, w.n_resources)
    lsc, lsh = _per_area(who, "load_scale", load_scale, n, 1.0), _per_area(who, "load_shift", load_shift, n, 0.0)
    st = _area_storages(who, storages, n)
    eng = engine or api.default_engine()
    t0 = time.time()
    hl1_areas._model_load(eng, units, cap, mttf, mttr, load, tf, tt, tc, kf, kr)
    _library_load(eng, w, n)
    opts = _abi.Hl1AreaVarOpts()
    for a in range(_abi.AREA_MAX):
        opts.load_scale[a], opts.load_shift[a] = (lsc[a], lsh[a]) if a < n else (1.0, 0.0)
    for r, v in enumerate(rs):
        opts.resource_scale[r] = v
    opts.policy, opts.flow, opts.pick, opts.reserved = int(policy), hl1_areas._FLOW[flow], _PICK[pick], 0
    arr = (_abi.Hl1AreaStorage * max(len(st), 1))()
    for i, s in enumerate(st):
        q = s.storage
        arr[i].s = _abi.Hl1Storage(float(q.charge_mw), float(q.discharge_mw), float(q.energy_mwh), float(q.eta_charge), float(q.eta_discharge), q.soc0)
        arr[i].area, arr[i].reserved = int(s.area) - 1, 0
    acc = (_abi.Hl1StorageAcc * (n + 1))()
    yr, sy, wy = np.zeros((n_years, n + 1, 3)), np.zeros((n_years, n + 1, 3)), np.zeros(n_years, dtype=np.int32)
    eng._check(eng.L.relmc_hl1_area_var(eng._h, int(seed), 0, chains, n_years // chains, hl1_areas._START[start], C.byref(opts), len(st),
                                        arr if st else None, acc, yr.ctypes.data_as(C.POINTER(_abi.Hl1SeqYear)),
                                        sy.ctypes.data_as(C.POINTER(_abi.Hl1StorageYear)), wy.ctypes.data_as(_abi.c_int32_p)), "relmc_hl1_area_var")
    per_year = lambda f: np.array([getattr(a, f) for a in acc]) / n_years
    lole, eue, lolf = per_year("sum_lole"), per_year("sum_eue"), per_year("sum_lolf")
    with np.errstate(invalid="ignore", divide="ignore"):
        lold = np.where(lolf > 0, lole / np.where(lolf > 0, lolf, 1.0), np.nan)
    return AreaVariableResult(policy, flow, [hl1_areas.AreaResult(a.name, float(lole[i]), float(eue[i])) for i, a in enumerate(sys.areas)],
                              lolf[:n].copy(), lold[:n].copy(), float(lole[n]), float(eue[n]), float(lolf[n]), float(lold[n]),
                              time.time() - t0, yr,
                              np.zeros(tf.size) if kf is None else np.where(np.isfinite(kf), kr / (np.where(np.isfinite(kf), kf, 1.0) + kr), 0.0),
                              served_hours=per_year("sum_served"), discharged_mwh=per_year("sum_discharged"), charged_mwh=per_year("sum_charged"),
                              year_storage=sy, year_weather=wy, resource_scale=rs, load_scale=lsc, load_shift=lsh, storages=st, pick=pick)


def area_variable_report(base: MultiAreaResult, result: AreaVariableResult) -> str:
    """LOLE and EUE of every area and of the system without (`base`: any MultiAreaResult of the same system) and with the resources and
    storages side by side, and what the storages of every area cycled per year."""
    rule = "-" * 86
    lines = ["", "=== AREA RESOURCES AND STORAGES (%s, %s) ===" % (result.policy.name, result.flow),
             "%-12s | %-12s %-12s | %-12s %-12s | %-9s %-10s" % ("Area", "LOLE before", "LOLE with", "EUE before", "EUE with", "served h", "MWh out/in"), rule]
    rows = [(b.area, b.lole, r.lole, b.eue, r.eue) for b, r in zip(base.results, result.results)]
    rows.append(("System", base.system_lole, result.system_lole, base.system_eue, result.system_eue))
    for i, (name, l0, l1, e0, e1) in enumerate(rows):
        lines.append("%-12s | %-12.4f %-12.4f | %-12.2f %-12.2f | %-9.4f %.2f / %.2f"
                     % (name, l0, l1, e0, e1, result.served_hours[i], result.discharged_mwh[i], result.charged_mwh[i]))
    lines.append(rule)
    n = sum(1 for v in result.resource_scale if v > 0.0)
    nw = np.unique(result.year_weather).size
    lines.append("%d resource%s, %d storage%s, %d weather year%s drawn (%s); storages act after the ties, each in its own area"
                 % (n, "" if n == 1 else "s", len(result.storages), "" if len(result.storages) == 1 else "s", nw, "" if nw == 1 else "s", result.pick))
    return "\n".join(lines) + "\n"


def area_resource_elcc(sys: System, weather, area: int, n_years: int, *, resources=(), storages=(), metric: str = "lole", row: str = "area",
                       bracket=None, rounds: int = 3, policy=hl1_areas.INTERCONNECTED, resource_scale=None, pick: str = "random",
                       flow: str = "max_flow", seed: int = 1, chains: int = 1, start: str = "all_up", engine=None) -> hl1.CarryingCapabilityResult:
    """What the resources `resources` (0-based indices into the library) and the storages `storages` (AreaStorage objects) are worth in
    load of area `area` (1-based): the shift of that area's load after which the system WITH them is as risky -- LOLE or EUE of that
    area (row="area") or of the system (row="system") -- as the system WITHOUT them (their scale 0, the storages removed) at the
    unshifted load, under the same seed, so both sides see the same unit, tie and weather history.  The other resources of the library
    are there on both sides.  Each round runs 8 equally spaced shifts over the bracket and keeps the FIRST adjacent pair that brackets
    the target; the last pair is interpolated linearly and the standard error comes from the per-year paired differences over the
    slope.  Only the system row under flow="max_flow" without storages is monotone in the shift (up to the solve's 1e-4 thresholds): no
    monotonicity is assumed, and ValueError is raised when no pair brackets.  The default bracket is (0, the largest summed scaled
    output of the chosen resources plus the storages' discharge_mw)."""
    who = "area_resource_elcc"
    n = len(sys.areas)
    if metric not in hl1_areas._AREA_METRIC:
        raise ValueError(f"{who}: metric must be one of {sorted(hl1_areas._AREA_METRIC)}, not {metric!r} (the sampled LOLF is not monotone)")
    if row not in ("area", "system"):
        raise ValueError(f"{who}: row must be 'area' or 'system', not {row!r}")
    if not (isinstance(area, (int, np.integer)) and 1 <= int(area) <= n):
        raise ValueError(f"{who}: area must be one of 1..{n} (1-based, as TieLine), not {area!r}")
    n_years, chains = hl1._seq_shape(who, n_years, chains, start)
    hours = {np.asarray(a.hourly_load).size for a in sys.areas}
    w = _area_weather(who, weather, n, hours.pop() if len(hours) == 1 else -1)
    rs = hl1_variable._resource_scale(who, resource_scale, w.n_resources)
    st = _area_storages(who, storages, n)
    chosen = sorted({int(r) for r in resources})
    if chosen and (chosen[0] < 0 or chosen[-1] >= w.n_resources):
        raise ValueError(f"{who}: resources must be indices in 0..{w.n_resources - 1}, not {chosen}")
    if not chosen and not st:
        raise ValueError(f"{who}: no resource and no storage given")
    top = float((np.asarray([rs[r] for r in chosen])[None, :, None] * w.output_mw[:, chosen, :]).sum(axis=1).max()) if chosen else 0.0
    top += sum(float(s.storage.discharge_mw) for s in st)
    if bracket is None and not top > 0.0:
        raise ValueError(f"{who}: the chosen resources and storages can deliver nothing")
    lo, hi, rounds = hl1._search_args(who, metric, "shift", (0.0, top) if bracket is None else bracket, rounds)
    t0 = time.time()
    a, q = int(area) - 1, hl1_areas._AREA_METRIC[metric]
    r_ = a if row == "area" else n
    kw = dict(pick=pick, flow=flow, seed=seed, chains=chains, start=start, engine=engine)
    without = tuple(0.0 if r in chosen else v for r, v in enumerate(rs))
    base = run_area_variable(sys, policy, w, n_years, resource_scale=without, **kw)
    target_year = base.year_indices[:, r_, q].copy()
    target = float(target_year.mean())
    for _ in range(rounds):
        x = np.linspace(lo, hi, 8)
        runs = [run_area_variable(sys, policy, w, n_years, storages=st, resource_scale=rs,
                                  load_shift=[float(v) if b == a else 0.0 for b in range(n)], **kw) for v in x]
        m = np.array([run.year_indices[:, r_, q].mean() for run in runs])
        i = _first_crossing(who, m, target)
        lo, hi = float(x[i]), float(x[i + 1])
    value, t, slope = _interpolate_pair(x, m, i, target)
    se_d = float(hl1._se((1.0 - t) * runs[i].year_indices[:, r_, q] + t * runs[i + 1].year_indices[:, r_, q] - target_year))
    return hl1.CarryingCapabilityResult("Multi-area sequential MC + resources", metric, "shift", value, se_d / abs(slope) if slope != 0 else float("inf"),
                                        (lo, hi), (float(m[i]), float(m[i + 1])), target, n_years, rounds, time.time() - t0, [target_year])


def synthetic_area_weather(sys: System, n_weather: int, *, solar_mw: float = 300.0, wind_mw: float = 300.0, seed: int = 2026,
                           load_curves: bool = False) -> AreaWeatherYears:
    """An ILLUSTRATIVE library for `sys`: hl1_variable.synthetic_weather's ("solar", "wind") pair for every area, each area from its own
    seed (seed + the area's index), nameplates solar_mw / wind_mw per area (at most 8 resources: four areas at most); with load_curves
    every area also gets that generator's per-weather-year load curves.  No measured data ships, and nothing here is fitted to any site."""
    n = len(sys.areas)
    if 2 * n > _abi.HL1_VAR_MAX_RESOURCES:
        raise ValueError(f"synthetic_area_weather: two resources per area need {2 * n} resources; {_abi.HL1_VAR_MAX_RESOURCES} at most")
    hours = int(np.asarray(sys.areas[0].hourly_load).size)
    libs = [hl1_variable.synthetic_weather(n_weather, hours, solar_mw, wind_mw, int(seed) + a,
                                           hl1.LoadModel(np.asarray(ar.hourly_load, dtype=np.float64)) if load_curves else None)
            for a, ar in enumerate(sys.areas)]
    out = np.concatenate([lib.output_mw for lib in libs], axis=1)
    curves = np.stack([lib.load_mw for lib in libs], axis=1) if load_curves else None
    names = tuple(f"{nm}_{ar.name}" for ar in sys.areas for nm in ("solar", "wind"))
    return AreaWeatherYears(out, tuple(a + 1 for a in range(n) for _ in range(2)), curves, names)
