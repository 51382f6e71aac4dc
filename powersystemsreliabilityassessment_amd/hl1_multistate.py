"""Units with a derated state on the HL1 sequential chronology — an extension beyond the reference (its units, PowerSystemAdequacy.jl:214-268,
and its Markov_process.jl are two-state).

A large thermal unit that loses a feed pump or a mill runs at part load for days.  The textbook treatment (Billinton & Allan) is a third,
DERATED state with its own capacity and transition rates: lumping it into DOWN overstates LOLE, ignoring it understates LOLE.  A unit here
is a continuous-time Markov chain over UP (0), DERATED (1) and DOWN (2); the library takes it as mean holding times and branch
probabilities (relmc_hl1_ms_load / relmc_hl1_ms_seq, the contract is written out in include/relmc.h), this module also as a rate matrix.

  MultiStateUnit(name, capacity, derated_capacity, rates)    one unit from its 3x3 per-hour rate matrix
  MultiStateUnit.from_generator(gen)                          a two-state hl1.Generator, mttf / mttr kept verbatim
  stationary(unit)                                            the long-run probabilities of the three states
  run_sequential_multistate(units, load, years)               run_sequential_mc's chronology with such units, on the GPU
  run_analytical_multistate(units, load, step_size)           the exact COPT, three terms per unit (host arithmetic)
  derated_rts24()                                             the RTS-24 fleet with its 350 MW and 400 MW units derated to half
"""
from __future__ import annotations

import ctypes as C
import math
import time
from dataclasses import dataclass, field

import numpy as np

from . import _abi, hl1

UP, DERATED, DOWN = 0, 1, 2
STATE_NAMES = ("UP", "DERATED", "DOWN")
DESTINATIONS = ((DOWN, DERATED), (UP, DOWN), (UP, DERATED))    # of each state: first-listed, other (include/relmc.h)
MAX_UNITS = 128


class MultiStateUnit:
    """One unit: `capacity` MW when UP, `derated_capacity` MW when DERATED, nothing when DOWN.  rates[i][j] is the transition rate from
    state i to state j per hour (the diagonal is ignored).  The library's form is kept beside it: mean_h[i] = 1 / (the sum of row i) and
    first_p[i] = the share of the first-listed destination (from UP: DOWN, from DERATED: UP, from DOWN: UP) in that sum.  A state
    whose row has no exit (an absorbing state; for UP, a unit that never fails) has no such form.  It is recorded in `no_exit`, with
    mean 1 and first_p 1 as placeholders that are never used: stationary() and the run_* functions refuse the unit when the state can
    be reached from UP (UP always can), and ignore the state otherwise, as the library ignores a state that is never entered."""

    def __init__(self, name, capacity: float, derated_capacity: float, rates):
        r = np.array(rates, dtype=np.float64)
        if r.shape != (3, 3):
            raise ValueError(f"MultiStateUnit {name!r}: rates must be a 3x3 matrix, not {r.shape}")
        np.fill_diagonal(r, 0.0)
        if not np.isfinite(r).all() or (r < 0).any():
            raise ValueError(f"MultiStateUnit {name!r}: rates must be finite and not negative")
        mean, first = [], []
        for i in range(3):
            out = r[i, DESTINATIONS[i][0]] + r[i, DESTINATIONS[i][1]]
            mean.append(1.0 / out if out > 0 else 1.0)
            first.append(r[i, DESTINATIONS[i][0]] / out if out > 0 else 1.0)
        self._set(name, capacity, derated_capacity, mean, first, tuple(not (r[i, DESTINATIONS[i][0]] + r[i, DESTINATIONS[i][1]] > 0) for i in range(3)))

    def _set(self, name, capacity, derated_capacity, mean_h, first_p, no_exit=(False, False, False)):
        self.name, self.capacity, self.derated_capacity = name, float(capacity), float(derated_capacity)
        self.mean_h, self.first_p = tuple(float(x) for x in mean_h), tuple(float(x) for x in first_p)
        self.no_exit = tuple(bool(x) for x in no_exit)       # states whose row of the rate matrix was all zero

    @classmethod
    def from_means(cls, name, capacity: float, derated_capacity: float, mean_h, first_p) -> "MultiStateUnit":
        """The library's form as it is: three mean holding times in hours and three first-destination probabilities."""
        if len(mean_h) != 3 or len(first_p) != 3:
            raise ValueError(f"MultiStateUnit {name!r}: mean_h and first_p have three entries each")
        u = cls.__new__(cls)
        u._set(name, capacity, derated_capacity, mean_h, first_p)
        return u

    @classmethod
    def from_generator(cls, gen: hl1.Generator) -> "MultiStateUnit":
        """A two-state unit: UP for mttf hours on average, DOWN for mttr, both verbatim, DERATED never reached.  A fleet of such units
        gives run_sequential_mc's year records bit for bit."""
        return cls.from_means(gen.id, gen.capacity, 0.0, (gen.mttf, 1.0, gen.mttr), (1.0, 1.0, 1.0))

    @property
    def rates(self) -> np.ndarray:
        r = np.zeros((3, 3))
        for i in range(3):
            a, b = DESTINATIONS[i]
            if not self.no_exit[i]:
                r[i, a], r[i, b] = self.first_p[i] / self.mean_h[i], (1.0 - self.first_p[i]) / self.mean_h[i]
        return r

    def __repr__(self):
        return f"MultiStateUnit({self.name!r}, {self.capacity}, {self.derated_capacity}, mean_h={self.mean_h}, first_p={self.first_p})"


def _chain(who: str, label: str, u: MultiStateUnit) -> tuple:
    """The library's checks of one unit, in its order, and the stationary start thresholds by its expressions:
    -> (reach[3], pi_2, pi_2 + pi_1, pi_1)."""
    vals = [u.capacity, u.derated_capacity, *u.mean_h, *u.first_p]
    if not all(math.isfinite(v) for v in vals):
        raise ValueError(f"{who}: a field of {label} is not finite")
    if not 0.0 <= u.derated_capacity <= u.capacity:
        raise ValueError(f"{who}: derated capacity of {label} not in [0, capacity]")
    reach, seen = [True, False, False], [False, False, False]
    while True:
        todo = [t for t in range(3) if reach[t] and not seen[t]]
        if not todo:
            break
        s = todo[0]
        seen[s] = True
        if u.no_exit[s]:                                      # a mean holding time the library would refuse: it is not finite
            raise ValueError(f"{who}: state {STATE_NAMES[s]} of {label} has no exit in its rate matrix" +
                             (" (the unit never fails)" if s == UP else f" and can be reached from UP: {label} cannot return to UP"))
        if not 0.0 <= u.first_p[s] <= 1.0:
            raise ValueError(f"{who}: first_p of state {STATE_NAMES[s]} of {label} not in [0, 1]")
        if not u.mean_h[s] > 0.0:
            raise ValueError(f"{who}: mean_h of state {STATE_NAMES[s]} of {label} not positive")
        if u.first_p[s] > 0.0:
            reach[DESTINATIONS[s][0]] = True
        if u.first_p[s] < 1.0:
            reach[DESTINATIONS[s][1]] = True
    f0, f1, f2 = u.first_p
    m = u.mean_h
    if reach[1] and reach[2]:
        if not (f1 > 0.0 or f2 > 0.0):
            raise ValueError(f"{who}: DERATED and DOWN of {label} cannot return to UP")
        nu0, nu1, nu2 = f2 + f1 * (1.0 - f2), (1.0 - f2) + f2 * (1.0 - f0), (1.0 - f1) + f1 * f0
        w0, w1, w2 = nu0 * m[0], nu1 * m[1], nu2 * m[2]
        tot = (w0 + w1) + w2
        pi2, pi1 = w2 / tot, w1 / tot
        return reach, pi2, pi2 + pi1, pi1
    if reach[2]:
        pi2 = m[2] / (m[0] + m[2])
        return reach, pi2, pi2, 0.0
    pi1 = m[1] / (m[0] + m[1])
    return reach, 0.0, pi1, pi1


def stationary(unit: MultiStateUnit) -> np.ndarray:
    """Long-run probabilities (UP, DERATED, DOWN) of a unit, by the library's expressions: proportional to nu_i * mean_h[i] with nu the
    stationary vector of the embedded jump chain over the states that can be reached from UP."""
    _, pi2, _, pi1 = _chain("stationary", f"unit {unit.name!r}", unit)
    return np.array([1.0 - pi1 - pi2, pi1, pi2])


def _units(who: str, units, limit=MAX_UNITS) -> list:
    """The checks of a fleet that need no device (the library's own, in its order)."""
    us = list(units)
    if not us:
        raise ValueError(f"{who}: no unit given")
    if limit is not None and len(us) > limit:
        raise ValueError(f"{who}: at most {limit} units, not {len(us)}")
    for i, u in enumerate(us):
        if not isinstance(u, MultiStateUnit):
            raise ValueError(f"{who}: unit {i} is not a MultiStateUnit (MultiStateUnit.from_generator converts a Generator)")
        _chain(who, f"unit {i}", u)
    return us


@dataclass
class MultiStateReliabilityResult(hl1.SequentialReliabilityResult):
    """run_sequential_multistate's result: run_sequential_mc's fields plus the unit-hours per year the fleet spent DERATED and DOWN
    (the per-year arrays in run_sequential_mc's order: chain-major)."""
    derated_unit_h_yr: float = 0.0
    down_unit_h_yr: float = 0.0
    year_derated: np.ndarray = field(default_factory=lambda: np.zeros(0))
    year_down: np.ndarray = field(default_factory=lambda: np.zeros(0))
    units: tuple = ()


def _load_array(who: str, load: hl1.LoadModel) -> np.ndarray:
    hl = np.ascontiguousarray(load.hourly_load, dtype=np.float64)
    if hl.ndim != 1 or hl.size < 1:
        raise ValueError(f"{who}: the load curve needs at least one hour")
    if hl.size > _abi.HL1_MS_MAX_HOURS:
        raise ValueError(f"{who}: more than 2^30 hours in the load curve")
    if not np.isfinite(hl).all():
        raise ValueError(f"{who}: load of hour {int(np.flatnonzero(~np.isfinite(hl))[0])} not finite")
    return hl


def _model_load(eng, us, hl: np.ndarray) -> None:
    """relmc_hl1_ms_load, unless this fleet and load curve are already on the device (they stay there between calls on the same model)."""
    arr = (_abi.Hl1MsUnit * len(us))(*[_abi.Hl1MsUnit(u.capacity, u.derated_capacity, (C.c_double * 3)(*u.mean_h), (C.c_double * 3)(*u.first_p))
                                       for u in us])
    key = (bytes(arr), hl.tobytes())
    if getattr(eng, "_hl1_ms_loaded", None) != key:
        eng._check(eng.L.relmc_hl1_ms_load(eng._h, len(us), arr, hl.size, hl.ctypes.data_as(_abi.c_double_p)), "relmc_hl1_ms_load")
        eng._hl1_ms_loaded = key


def run_sequential_multistate(units, load: hl1.LoadModel, years: int, *, seed: int = 1, chains: int = 1, start: str = "all_up",
                              engine=None) -> MultiStateReliabilityResult:
    """run_sequential_mc's chronology (same arguments, same draws for the durations) with MultiStateUnit units, at most 128.
    start="stationary" draws each unit's start state from stationary(unit).  A fleet of MultiStateUnit.from_generator units gives
    run_sequential_mc's per-year arrays bit for bit.  The result goes into hl1.compare_results like any other."""
    from . import api
    who = "run_sequential_multistate"
    years, chains = hl1._seq_shape(who, years, chains, start)
    us = _units(who, units)
    hl = _load_array(who, load)
    eng = engine or api.default_engine()
    t0 = time.time()
    _model_load(eng, us, hl)
    acc = _abi.Hl1MsAcc()
    yr, sy = np.zeros((years, 3)), np.zeros((years, 2))
    eng._check(eng.L.relmc_hl1_ms_seq(eng._h, int(seed), 0, chains, years // chains, hl1._SEQ_START[start], C.byref(acc),
                                      yr.ctypes.data_as(C.POINTER(_abi.Hl1SeqYear)), sy.ctypes.data_as(C.POINTER(_abi.Hl1MsYear))),
               "relmc_hl1_ms_seq")
    k = np.arange(10, years + 1, 10)
    history = np.cumsum(yr[:, 0])[k - 1] / k if k.size else np.zeros(0)
    lole, eue, lolf = acc.sum_lole / years, acc.sum_eue / years, acc.sum_lolf / years
    return MultiStateReliabilityResult("Sequential MC 3-state", lole, eue, time.time() - t0, history, lolf_occ_yr=lolf,
                                       lold_hours=lole / lolf if lolf > 0 else float("nan"),
                                       year_lole=yr[:, 0].copy(), year_eue=yr[:, 1].copy(), year_lolf=yr[:, 2].copy(),
                                       derated_unit_h_yr=acc.sum_derated / years, down_unit_h_yr=acc.sum_down / years,
                                       year_derated=sy[:, 0].copy(), year_down=sy[:, 1].copy(), units=tuple(us))


def _shifted(probs: np.ndarray, k: int, n_new: int) -> np.ndarray:
    out = np.zeros(n_new)
    if k < n_new:
        m = min(probs.size, n_new - k)
        out[k:k + m] = probs[:m]
    return out


def _outage_term(probs: np.ndarray, outage_mw: float, p: float, step_size: float, n_new: int) -> np.ndarray:
    """probs shifted by an outage of outage_mw with probability p, the capacity rounding split between the neighbouring steps as
    hl1.convolve_unit splits it."""
    lower = int(np.floor(outage_mw / step_size))
    if abs(outage_mw - lower * step_size) < 1e-5:
        return _shifted(probs, lower, n_new) * p
    alpha = (outage_mw - lower * step_size) / step_size
    return _shifted(probs, lower, n_new) * (p * (1.0 - alpha)) + _shifted(probs, lower + 1, n_new) * (p * alpha)


def convolve_multistate_unit(probs: np.ndarray, unit: MultiStateUnit, step_size: float) -> np.ndarray:
    """The COPT recursion for one unit, `probs[k]` = P(outage = k * step_size): nothing out with pi_0, capacity - derated_capacity out with
    pi_1, capacity out with pi_2.  A unit that never derates takes hl1.convolve_unit's two terms."""
    pi = stationary(unit)
    if pi[1] == 0.0:
        return hl1.convolve_unit(probs, unit.capacity, float(pi[2]), step_size)
    max_old = (probs.size - 1) * step_size if probs.size else 0.0
    n_new = int(np.ceil((max_old + unit.capacity) / step_size)) + 1
    return (_shifted(probs, 0, n_new) * pi[0] + _outage_term(probs, unit.capacity - unit.derated_capacity, pi[1], step_size, n_new)
            + _outage_term(probs, unit.capacity, pi[2], step_size, n_new))


def run_analytical_multistate(units, load: hl1.LoadModel, step_size: float = 10.0) -> hl1.ReliabilityResult:
    """Exact (up to the capacity step) stationary LOLE / EUE by convolution, hl1.run_analytical with three terms per unit; for two-state
    units it gives run_analytical's numbers."""
    who = "run_analytical_multistate"
    us = _units(who, units, limit=None)                        # host arithmetic: any number of units
    if not step_size > 0:
        raise ValueError(f"{who}: step_size must be positive")
    t0 = time.time()
    probs = np.array([1.0])
    for u in us:
        probs = convolve_multistate_unit(probs, u, step_size)
    outage = np.arange(probs.size) * step_size
    installed = sum(u.capacity for u in us)
    cum = np.cumsum(probs[::-1])[::-1]                         # P(outage >= X)
    tail_w = np.cumsum((outage * probs)[::-1])[::-1]           # sum_{k>=i} outage_k p_k
    lole = eue = 0.0
    for load_mw in np.asarray(load.hourly_load, dtype=float):  # hl1.run_analytical's sweep of the load curve
        reserve = installed - load_mw
        idx = int(np.floor(reserve / step_size)) + 1
        if 0 <= idx < probs.size:
            lole += cum[idx]
            eue += tail_w[idx] - reserve * cum[idx]
        elif idx < 0:
            lole += 1.0
            eue += (load_mw - installed) + float(outage @ probs)
    return hl1.ReliabilityResult("Analytical 3-state", lole, eue, time.time() - t0)


def derated_rts24() -> list:
    """The RTS-24 fleet (hl1.rts24_generators) in which the 350 MW unit and the two 400 MW units have a DERATED state at half capacity;
    every other unit stays two-state with its mttf / mttr verbatim.

    The derated rates are ILLUSTRATIVE, not published data: they are built from the unit's own failure rate l = 1 / mttf and repair
    rate m = 1 / mttr so that every branch is taken,
        UP -> DERATED  l        UP -> DOWN       l
        DERATED -> UP  2 m      DERATED -> DOWN  0.2 m
        DOWN -> UP     m        DOWN -> DERATED  0.25 m
    i.e. a partial outage is as frequent as a full one, is repaired twice as fast, now and then grows into a full outage, and a fifth
    of the repairs bring the unit back at half load first."""
    out = []
    for g in hl1.rts24_generators():
        if g.capacity in (350.0, 400.0):
            l, m = 1.0 / g.mttf, 1.0 / g.mttr
            out.append(MultiStateUnit(g.id, g.capacity, 0.5 * g.capacity, [[0.0, l, l], [2.0 * m, 0.0, 0.2 * m], [m, 0.25 * m, 0.0]]))
        else:
            out.append(MultiStateUnit.from_generator(g))
    return out
