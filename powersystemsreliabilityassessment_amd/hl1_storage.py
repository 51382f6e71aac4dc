"""Energy storage on the HL1 sequential chronology — an extension beyond the reference (its only energy-limited resource, the ELU of
hl1_planning.py, drains and never recharges, on an hourly-sampling Monte Carlo).

A storage's state of charge couples the hours, so its effect on LOLE, EUE and LOLF exists only on a chronology: the storages discharge
into a shortfall of the fleet and charge from its surplus generation, in the order they are given (relmc_hl1_seq_storage; the step rule
is written out in include/relmc.h).

  Storage(charge_mw, discharge_mw, energy_mwh, ...)         one storage; it never fails
  run_sequential_storage(gens, load, storages, years)        run_sequential_mc's chronology with the storages, on the GPU
  storage_report(base, with_storage)                         the indices without and with storage side by side (text)
  storage_elcc(gens, load, storages, years)                  what the storages are worth in load (hl1.CarryingCapabilityResult)
"""
from __future__ import annotations

import ctypes as C
import math
import time
from dataclasses import dataclass, field

import numpy as np

from . import _abi, hl1
from .hl1_areas import _first_crossing, _interpolate_pair


@dataclass(frozen=True)
class Storage:
    """One energy storage: power limits in MW, energy capacity in MWh, one-way efficiencies in (0, 1] (charging y MW for an hour stores
    y * eta_charge MWh; delivering x MW for an hour takes x / eta_discharge MWh), and the state of charge at the start of every chain
    (None: full)."""
    charge_mw: float
    discharge_mw: float
    energy_mwh: float
    eta_charge: float = 1.0
    eta_discharge: float = 1.0
    soc0_mwh: float = None

    @property
    def soc0(self) -> float:
        return float(self.energy_mwh if self.soc0_mwh is None else self.soc0_mwh)


@dataclass
class StorageReliabilityResult(hl1.SequentialReliabilityResult):
    """run_sequential_storage's result: run_sequential_mc's fields for the hours left after storage, plus what the storages did per year
    (the per-year arrays in run_sequential_mc's order: chain-major)."""
    served_hours_yr: float = 0.0      # short hours the storages covered in full (served + LOLE = the LOLE without storage)
    discharged_mwh_yr: float = 0.0    # energy delivered to the load
    charged_mwh_yr: float = 0.0       # surplus generation taken
    year_served: np.ndarray = field(default_factory=lambda: np.zeros(0))
    year_discharged: np.ndarray = field(default_factory=lambda: np.zeros(0))
    year_charged: np.ndarray = field(default_factory=lambda: np.zeros(0))
    storages: tuple = ()
    scale: float = 1.0
    shift: float = 0.0


def _storages(who: str, storages) -> tuple:
    """The checks of the storages that need no device (the library's own, in its order); returns a tuple of Storage."""
    st = tuple(x if isinstance(x, Storage) else Storage(*x) for x in storages)
    if len(st) > _abi.HL1_MAX_STORAGE:
        raise ValueError(f"{who}: at most {_abi.HL1_MAX_STORAGE} storages, not {len(st)}")
    for i, s in enumerate(st):
        vals = {"charge_mw": s.charge_mw, "discharge_mw": s.discharge_mw, "energy_mwh": s.energy_mwh, "eta_charge": s.eta_charge,
                "eta_discharge": s.eta_discharge, "soc0_mwh": s.soc0}
        for name, v in vals.items():
            if not math.isfinite(float(v)):
                raise ValueError(f"{who}: {name} of storage {i} not finite")
        for name in ("charge_mw", "discharge_mw", "energy_mwh"):
            if vals[name] < 0:
                raise ValueError(f"{who}: {name} of storage {i} is negative")
        for name in ("eta_charge", "eta_discharge"):
            if not 0.0 < vals[name] <= 1.0:
                raise ValueError(f"{who}: {name} of storage {i} not in (0, 1]")
        if not 0.0 <= s.soc0 <= s.energy_mwh:
            raise ValueError(f"{who}: soc0_mwh of storage {i} not in [0, energy_mwh]")
    return st


def _level(who: str, scale, shift) -> tuple:
    scale, shift = float(scale), float(shift)
    if not (math.isfinite(scale) and math.isfinite(shift)):
        raise ValueError(f"{who}: scale / shift not finite")
    return scale, shift


def run_sequential_storage(gens, load: hl1.LoadModel, storages, years: int, *, scale: float = 1.0, shift: float = 0.0, seed: int = 1,
                           chains: int = 1, start: str = "all_up", engine=None) -> StorageReliabilityResult:
    """run_sequential_mc's chronology (same arguments, same chains under the same seed) at the load scale * load + shift with the storages
    `storages` (Storage objects or their field tuples, at most 8, used in the order given).  Without storages the per-year arrays are
    run_sequential_mc's bit for bit."""
    from . import api
    who = "run_sequential_storage"
    years, chains = hl1._seq_shape(who, years, chains, start)
    st = _storages(who, storages)
    scale, shift = _level(who, scale, shift)
    eng = engine or api.default_engine()
    t0 = time.time()
    hl1._seq_model_load(eng, gens, load)
    arr = (_abi.Hl1Storage * max(len(st), 1))(*[_abi.Hl1Storage(float(s.charge_mw), float(s.discharge_mw), float(s.energy_mwh),
                                                                 float(s.eta_charge), float(s.eta_discharge), s.soc0) for s in st])
    acc = _abi.Hl1StorageAcc()
    yr, sy = np.zeros((years, 3)), np.zeros((years, 3))
    eng._check(eng.L.relmc_hl1_seq_storage(eng._h, int(seed), 0, chains, years // chains, hl1._SEQ_START[start], scale, shift, len(st),
                                           arr if st else None, C.byref(acc), yr.ctypes.data_as(C.POINTER(_abi.Hl1SeqYear)),
                                           sy.ctypes.data_as(C.POINTER(_abi.Hl1StorageYear))), "relmc_hl1_seq_storage")
    k = np.arange(10, years + 1, 10)
    history = np.cumsum(yr[:, 0])[k - 1] / k if k.size else np.zeros(0)
    lole, eue, lolf = acc.sum_lole / years, acc.sum_eue / years, acc.sum_lolf / years
    return StorageReliabilityResult("Sequential MC + storage" if st else "Sequential MC", lole, eue, time.time() - t0, history,
                                    lolf_occ_yr=lolf, lold_hours=lole / lolf if lolf > 0 else float("nan"),
                                    year_lole=yr[:, 0].copy(), year_eue=yr[:, 1].copy(), year_lolf=yr[:, 2].copy(),
                                    served_hours_yr=acc.sum_served / years, discharged_mwh_yr=acc.sum_discharged / years,
                                    charged_mwh_yr=acc.sum_charged / years, year_served=sy[:, 0].copy(), year_discharged=sy[:, 1].copy(),
                                    year_charged=sy[:, 2].copy(), storages=st, scale=scale, shift=shift)


def storage_report(base: hl1.SequentialReliabilityResult, with_storage: StorageReliabilityResult) -> str:
    """LOLE, EUE and LOLF without and with storage side by side, the hours served and the MWh cycled per year, in compare_results' style."""
    rule = "=" * 42
    lines = [rule, "         STORAGE SUMMARY", rule,
             "%-24s | %-10s | %-10s | %-12s" % ("Method", "LOLE(h/yr)", "EUE(MWh)", "LOLF(occ/yr)"), "-" * 66]
    lines += ["%-24s | %-10.4f | %-10.2f | %-12.4f" % (r.method, r.lole_hours_yr, r.eue_mwh_yr, r.lolf_occ_yr) for r in (base, with_storage)]
    lines.append("-" * 66)
    s = with_storage
    lines.append("%d storage%s: %.4f short hours/yr served in full, %.2f MWh/yr delivered, %.2f MWh/yr of surplus taken"
                 % (len(s.storages), "" if len(s.storages) == 1 else "s", s.served_hours_yr, s.discharged_mwh_yr, s.charged_mwh_yr))
    return "\n".join(lines) + "\n"


def storage_elcc(gens, load: hl1.LoadModel, storages, years: int, *, metric: str = "lole", bracket=None, rounds: int = 3, seed: int = 1,
                 chains: int = 1, start: str = "all_up", engine=None) -> hl1.CarryingCapabilityResult:
    """What the storages are worth in load: the load shift in MW after which the fleet with the storages is as risky as the fleet without
    them at the unshifted load.  The target is run_sequential_mc's metric under the same seed, chains and start.  Each round evaluates 8
    equally spaced shifts with the storages under that seed and keeps the first adjacent pair that brackets the target; the last pair
    is interpolated linearly.  The storages deliver at most the sum of their discharge_mw in any hour, so the default bracket
    (0, that sum) holds the root.  With one storage the sampled metric is monotone in the shift (a higher state of charge and a higher
    margin give a higher state of charge and a lower deficit at every step); with several no monotonicity is claimed, and ValueError is
    raised when no pair brackets.  Both runs see the same fleet history, so the standard error comes from the per-year paired
    differences between the interpolated pair and the target, over the slope."""
    who = "storage_elcc"
    years, chains = hl1._seq_shape(who, years, chains, start)
    st = _storages(who, storages)
    if not st:
        raise ValueError(f"{who}: no storage given")
    default = (0.0, float(sum(s.discharge_mw for s in st)))
    lo, hi, rounds = hl1._search_args(who, metric, "shift", default if bracket is None else bracket, rounds)
    t0 = time.time()
    kw = dict(seed=seed, chains=chains, start=start, engine=engine)
    per_year, attr = "year_" + metric, hl1._SWEEP_METRIC[metric]
    base = hl1.run_sequential_mc(gens, load, years, **kw)
    target, target_year = float(getattr(base, attr)), getattr(base, per_year)
    for _ in range(rounds):
        x = np.linspace(lo, hi, 8)
        runs = [run_sequential_storage(gens, load, st, years, shift=float(v), **kw) for v in x]
        m = np.array([getattr(r, attr) for r in runs])
        i = _first_crossing(who, m, target)
        lo, hi = float(x[i]), float(x[i + 1])
    value, t, slope = _interpolate_pair(x, m, i, target)
    se_d = float(hl1._se((1.0 - t) * getattr(runs[i], per_year) + t * getattr(runs[i + 1], per_year) - target_year))
    return hl1.CarryingCapabilityResult("Sequential MC + storage", metric, "shift", value, se_d / abs(slope) if slope != 0 else float("inf"),
                                        (lo, hi), (float(m[i]), float(m[i + 1])), target, years, rounds, time.time() - t0, [target_year.copy()])
