"""Loss attribution on the HL1 sequential chronology: which units are down when load is lost, and what each unit's unreliability costs.

The reference ends both Monte Carlo drivers with a component ranking, comp_importance = the share of the failed samples (nsqMain.m:366-376)
or of the loss hours (seqMain.m:144-158, 233) in which a component was out.  relmc_hl1_attr_seq (the contract is written out in
include/relmc.h) does that for run_sequential_mc's chronology: every loss step of a chain is charged to the units that are DOWN in it.
Because the units are independent, two of the charged quantities are exact counterfactuals on the same fleet history: the loss hours and
the energy that would not have been lost with unit k always UP.  One walk of the chains gives them for every unit.

  run_sequential_attribution(generators, load, n_years)   the indices of run_sequential_mc and, per unit, importance, energy_importance,
                                                          lole_if_perfect and eue_if_perfect with standard errors over the chains
  run_analytical_attribution(generators, load)            their exact stationary counterparts from the COPT of the fleet without unit k
  attribution_report(mc, analytical=None)                 the ranked table (text)
"""
from __future__ import annotations

import ctypes as C
import time
from dataclasses import dataclass

import numpy as np

from . import _abi, hl1

FIELDS = ("down_hours", "down_mwh", "critical_hours", "relief_mwh")      # relmc_hl1_attr_unit, in order


@dataclass
class AttributionResult:
    """run_sequential_attribution's result.  Index k is generators[k].  The per-unit means are per simulated year; the standard errors are
    over the chains (NaN with one chain), those of the two importances by the delta method for a ratio of chain means."""
    years: int
    chains: int
    lole_hours_yr: float
    eue_mwh_yr: float
    lolf_occ_yr: float
    lole_se: float
    eue_se: float
    down_hours_yr: np.ndarray         # loss hours per year with unit k DOWN
    down_mwh_yr: np.ndarray           # their unserved energy
    critical_hours_yr: np.ndarray     # loss hours per year that unit k, UP, would have prevented
    relief_mwh_yr: np.ndarray         # unserved energy per year that unit k, UP, would have served
    down_hours_se: np.ndarray
    down_mwh_se: np.ndarray
    critical_hours_se: np.ndarray
    relief_mwh_se: np.ndarray
    importance: np.ndarray            # down_hours / loss hours: the reference's comp_importance (seqMain.m:233)
    importance_se: np.ndarray
    energy_importance: np.ndarray     # down_mwh / EUE
    energy_importance_se: np.ndarray
    lole_if_perfect: np.ndarray       # LOLE - critical_hours / years: the LOLE with unit k perfectly reliable, on the same history
    lole_if_perfect_se: np.ndarray
    eue_if_perfect: np.ndarray        # EUE - relief_mwh / years
    eue_if_perfect_se: np.ndarray
    year_lole: np.ndarray             # [years], chain-major as run_sequential_mc's
    year_eue: np.ndarray
    year_lolf: np.ndarray
    unit_records: np.ndarray          # [chains, units, 4]: every chain's record in FIELDS' order
    computation_time: float


@dataclass
class AnalyticalAttribution:
    """run_analytical_attribution's result: the exact stationary expectations per year, index k = generators[k]."""
    lole_hours_yr: float
    eue_mwh_yr: float
    down_hours_yr: np.ndarray
    down_mwh_yr: np.ndarray
    critical_hours_yr: np.ndarray
    relief_mwh_yr: np.ndarray
    importance: np.ndarray
    energy_importance: np.ndarray
    lole_if_perfect: np.ndarray
    eue_if_perfect: np.ndarray
    computation_time: float


def _curve(who: str, load: hl1.LoadModel, scale, shift) -> np.ndarray:
    scale, shift = float(scale), float(shift)
    if not (np.isfinite(scale) and np.isfinite(shift)):
        raise ValueError(f"{who}: scale / shift not finite")
    return np.float64(scale) * np.asarray(load.hourly_load, dtype=np.float64) + np.float64(shift)


def _ratio(num: np.ndarray, den: np.ndarray) -> tuple:
    """mean(num) / mean(den) per unit with its delta-method standard error; num[chains, units], den[chains].  NaN without a loss."""
    n = den.size
    mn, md = num.mean(axis=0), float(den.mean())
    if md == 0.0:
        nan = np.full(num.shape[1], np.nan)
        return nan, nan.copy()
    r = mn / md
    if n < 2:
        return r, np.full(num.shape[1], np.nan)
    resid = num - r[None, :] * den[:, None]
    return r, resid.std(axis=0, ddof=1) / np.sqrt(n) / md


def run_sequential_attribution(generators, load: hl1.LoadModel, n_years: int, *, chains: int = 1, start: str = "all_up", seed: int = 1,
                               scale: float = 1.0, shift: float = 0.0, engine=None) -> AttributionResult:
    """run_sequential_mc's chronology (same arguments, same chains under the same seed) against the load scale * load + shift, with every
    loss step charged to the units that are DOWN in it.  The year records are run_sequential_mc's bit for bit at the default scale and
    shift.  lole_if_perfect[k] and eue_if_perfect[k] are what the same fleet history gives with unit k always UP: exact differences, not
    a second run, so they are never above LOLE and EUE (for a unit of non-negative capacity)."""
    from . import api
    who = "run_sequential_attribution"
    years, chains = hl1._seq_shape(who, n_years, chains, start)
    if len(generators) < 1:
        raise ValueError(f"{who}: no generators")
    _curve(who, load, scale, shift)
    eng = engine or api.default_engine()
    t0 = time.time()
    hl1._seq_model_load(eng, generators, load)
    K, ypc = len(generators), years // chains
    acc = _abi.Hl1SeqAcc()
    uacc = (_abi.Hl1AttrAcc * K)()
    yr = np.zeros((years, 3))
    rec = np.zeros((chains, K, 4))
    eng._check(eng.L.relmc_hl1_attr_seq(eng._h, int(seed), 0, chains, ypc, hl1._SEQ_START[start], float(scale), float(shift), C.byref(acc),
                                        yr.ctypes.data_as(C.POINTER(_abi.Hl1SeqYear)), uacc, rec.ctypes.data_as(C.POINTER(_abi.Hl1AttrUnit))),
               "relmc_hl1_attr_seq")
    lole, eue, lolf = acc.sum_lole / years, acc.sum_eue / years, acc.sum_lolf / years
    s1 = np.array([list(a.sum) for a in uacc])                   # [units, 4]
    s2 = np.array([list(a.sum2) for a in uacc])
    mean = s1 / years                                            # per simulated year
    if chains > 1:                                               # standard error of the chain mean, per year of a chain
        var = np.maximum(s2 - s1 * s1 / chains, 0.0) / (chains - 1)
        se = np.sqrt(var / chains) / ypc
    else:
        se = np.full((K, 4), np.nan)
    chain_l = yr[:, 0].reshape(chains, ypc).sum(axis=1)
    chain_e = yr[:, 1].reshape(chains, ypc).sum(axis=1)
    imp, imp_se = _ratio(rec[:, :, 0], chain_l)
    eimp, eimp_se = _ratio(rec[:, :, 1], chain_e)
    lip = (chain_l[:, None] - rec[:, :, 2]) / ypc                 # per chain: LOLE of the history with unit k always UP
    eip = (chain_e[:, None] - rec[:, :, 3]) / ypc
    return AttributionResult(years, chains, lole, eue, lolf, float(hl1._se(chain_l / ypc)), float(hl1._se(chain_e / ypc)),
                             mean[:, 0], mean[:, 1], mean[:, 2], mean[:, 3], se[:, 0], se[:, 1], se[:, 2], se[:, 3],
                             imp, imp_se, eimp, eimp_se, lole - mean[:, 2], hl1._se(lip.T), eue - mean[:, 3], hl1._se(eip.T),
                             yr[:, 0].copy(), yr[:, 1].copy(), yr[:, 2].copy(), rec, time.time() - t0)


def run_analytical_attribution(generators, load: hl1.LoadModel, *, scale: float = 1.0, shift: float = 0.0,
                               step_size: float = 1.0) -> AnalyticalAttribution:
    """The exact stationary counterparts.  With A_-k the available capacity of the fleet without unit k (its COPT: hl1.run_analytical on
    that fleet), q_k the unit's forced outage rate and c_k its capacity, per year
        E[down_hours_k]     = q_k sum_h P(A_-k < L_h)                       = q_k LOLE_-k(L)
        E[critical_hours_k] = q_k sum_h P(L_h - c_k <= A_-k < L_h)          = q_k (LOLE_-k(L) - LOLE_-k(L - c_k))
        E[down_mwh_k]       = q_k sum_h E[(L_h - A_-k)+]                    = q_k EUE_-k(L)
        E[relief_mwh_k]     = q_k sum_h E[min((L_h - A_-k)+, c_k)]          = q_k (EUE_-k(L) - EUE_-k(L - c_k))
    since unit k is DOWN independently of the others.  Exact up to the COPT's capacity step (exact for capacities that are multiples of
    step_size); capacities are taken as non-negative."""
    t0 = time.time()
    who = "run_analytical_attribution"
    curve = _curve(who, load, scale, shift)
    if len(generators) < 1:
        raise ValueError(f"{who}: no generators")
    if any(g.capacity < 0 for g in generators):
        raise ValueError(f"{who}: negative capacity")
    base = hl1.run_analytical(generators, hl1.LoadModel(curve), step_size=step_size)
    K = len(generators)
    out = np.zeros((K, 4))
    for k, g in enumerate(generators):
        rest = [x for i, x in enumerate(generators) if i != k]
        at = hl1.run_analytical(rest, hl1.LoadModel(curve), step_size=step_size)
        below = hl1.run_analytical(rest, hl1.LoadModel(curve - g.capacity), step_size=step_size)
        q = g.for_rate
        out[k] = (q * at.lole_hours_yr, q * at.eue_mwh_yr, q * (at.lole_hours_yr - below.lole_hours_yr), q * (at.eue_mwh_yr - below.eue_mwh_yr))
    lole, eue = base.lole_hours_yr, base.eue_mwh_yr
    nan = np.full(K, np.nan)
    return AnalyticalAttribution(lole, eue, out[:, 0], out[:, 1], out[:, 2], out[:, 3], out[:, 0] / lole if lole > 0 else nan,
                                 out[:, 1] / eue if eue > 0 else nan.copy(), lole - out[:, 2], eue - out[:, 3], time.time() - t0)


def attribution_report(mc: AttributionResult, analytical: AnalyticalAttribution = None) -> str:
    """The units ranked by importance (ties and runs without a loss: by unit index): importance and energy importance, LOLE and EUE with
    the unit perfectly reliable, each with its standard error, and with `analytical` the exact importance and LOLE-if-perfect beside them."""
    key = np.where(np.isnan(mc.importance), -1.0, mc.importance)
    order = sorted(range(key.size), key=lambda k: (-key[k], k))
    rule = "=" * 42
    head = "%-4s | %-4s | %-20s | %-20s | %-24s | %-24s" % ("Rank", "Unit", "Importance +- SE", "Energy imp. +- SE", "LOLE if perfect +- SE",
                                                          "EUE if perfect +- SE")
    if analytical is not None:
        head += " | %-10s | %-13s" % ("Imp. exact", "LOLE-if exact")
    lines = [rule, "       LOSS ATTRIBUTION SUMMARY", rule,
             "LOLE %.4f +- %.4f h/yr, EUE %.2f +- %.2f MWh/yr, %d years in %d chains" % (mc.lole_hours_yr, mc.lole_se, mc.eue_mwh_yr, mc.eue_se,
                                                                                        mc.years, mc.chains), head, "-" * len(head)]
    for rank, k in enumerate(order, 1):
        row = "%-4d | %-4d | %-9.4f +- %-7.4f | %-9.4f +- %-7.4f | %-11.4f +- %-9.4f | %-11.2f +- %-9.2f" % (
            rank, k, mc.importance[k], mc.importance_se[k], mc.energy_importance[k], mc.energy_importance_se[k],
            mc.lole_if_perfect[k], mc.lole_if_perfect_se[k], mc.eue_if_perfect[k], mc.eue_if_perfect_se[k])
        if analytical is not None:
            row += " | %-10.4f | %-13.4f" % (analytical.importance[k], analytical.lole_if_perfect[k])
        lines.append(row)
    lines.append("-" * len(head))
    return "\n".join(lines) + "\n"
