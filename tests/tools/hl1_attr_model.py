"""Host model of the loss attribution on the HL1 sequential chronology (relmc_hl1_attr_seq, include/relmc.h).

Built on hl1_seq_model.chronology (the draws and the transition times).  Per chain and unit k, over the chain's steps n = 1 .. Y*H that are
loss steps (cap_avail < L, L = scale * load[h] + shift with product and sum each rounded) with unit k DOWN:
    down_hours, down_mwh = sum of d = L - cap_avail, critical_hours = #{!(cap_avail + cap_k < L)}, relief_mwh = sum of fmin(d, cap_k).
The two fp64 sums are ONE accumulator per unit, added in ascending step order over the whole chain: attr_chain adds them in a Python loop
over the loss steps (sequential sums, not np.sum, whose pairwise order is another), so the device is compared bit for bit.

  attr_chain(down0, T, cap, L_year, years)   one chain -> (year records (lole, eue, lolf), unit records [K, 4])
  attr_model(seed, chains, cap, mttf, mttr, load, years, start, scale, shift)
                                             -> (lole, eue, lolf) chain-major as hl1_seq_model.interval_model, units[nchains, K, 4]
  brute_chain(...)                           the same by a literal hour loop over a unit-state table (for the model's own test)
"""
from __future__ import annotations

import importlib.util
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("hl1_seq_model", os.path.join(_HERE, "hl1_seq_model.py"))
SEQ = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(SEQ)


def level_load(load, scale: float = 1.0, shift: float = 0.0) -> np.ndarray:
    """scale * load + shift, the product and the sum each rounded (two numpy operations)."""
    return np.float64(scale) * np.asarray(load, dtype=np.float64) + np.float64(shift)


def down_table(down0, T, nsteps: int) -> np.ndarray:
    """down[k, n - 1]: unit k is DOWN at step n = its start state toggled once per T_j <= n."""
    n = np.arange(1, nsteps + 1, dtype=np.float64)
    out = np.zeros((len(down0), nsteps), dtype=bool)
    for k in range(len(down0)):
        cnt = np.searchsorted(T[k], n, side="right")
        out[k] = bool(down0[k]) ^ (cnt & 1).astype(bool)
    return out


def attr_chain(down0, T, cap, L_year, years: int):
    """One chain: down0[K], T[K, E], the year's load L_year[H] (already scaled and shifted).  Returns ((lole, eue, lolf)[years] each,
    units[K, 4]).  The year EUE is summed as hl1_seq_model.interval_chain sums it (the device's lane order differs: the tests compare it
    bitwise with the device's own sequential kernel, not with this)."""
    cap = np.asarray(cap, dtype=np.float64)
    L_year = np.asarray(L_year, dtype=np.float64)
    H = L_year.size
    S = years * H
    down = down_table(down0, T, S)
    cav = np.zeros(S)
    for k in range(cap.size):                                      # ascending unit order, + 0.0 for a DOWN unit (exact)
        cav = cav + np.where(down[k], 0.0, float(cap[k]))
    ld = np.tile(L_year, years)
    loss = cav < ld
    deficit = np.where(loss, ld - cav, 0.0)
    rise = loss & ~np.concatenate([[False], loss[:-1]])
    yrs = (loss.reshape(years, H).sum(1).astype(np.float64), deficit.reshape(years, H).sum(1), rise.reshape(years, H).sum(1).astype(np.float64))
    units = np.zeros((cap.size, 4))
    steps = np.flatnonzero(loss)                                   # ascending
    for k in range(cap.size):
        ck = float(cap[k])
        hours = crit = 0
        mwh = relief = 0.0
        for n in steps[down[k, steps]].tolist():                  # sequential sums in step order
            d, c, l = float(deficit[n]), float(cav[n]), float(ld[n])
            hours += 1
            mwh += d
            crit += 0 if (c + ck < l) else 1
            relief += min(d, ck)
        units[k] = (hours, mwh, crit, relief)
    return yrs, units


def attr_model(seed: int, chains, cap, mttf, mttr, load, years: int, start: int, scale: float = 1.0, shift: float = 0.0):
    chains = np.atleast_1d(np.asarray(chains, dtype=np.uint64))
    L_year = level_load(load, scale, shift)
    H = L_year.size
    lole, eue, lolf, units = [], [], [], []
    for c0 in range(0, chains.size, 256):
        down0, T, _ = SEQ.chronology(seed, chains[c0:c0 + 256], mttf, mttr, start, years * H)
        for c in range(down0.shape[0]):
            (a, b, f), u = attr_chain(down0[c], T[c], cap, L_year, years)
            lole.append(a); eue.append(b); lolf.append(f); units.append(u)
    return (np.concatenate(lole), np.concatenate(eue), np.concatenate(lolf)), np.stack(units)


def brute_chain(seed: int, chain: int, cap, mttf, mttr, load, years: int, start: int, scale: float = 1.0, shift: float = 0.0):
    """A literal loop over the hours and, inside it, over the units, on states read off the transition times one step at a time:
    -> units[K, 4].  Shares only the draws with attr_chain."""
    cap = [float(x) for x in cap]
    K = len(cap)
    L_year = [float(x) for x in level_load(load, scale, shift)]
    H = len(L_year)
    down0, T, _ = SEQ.chronology(seed, [chain], mttf, mttr, start, years * H)
    Tl = [T[0][k].tolist() for k in range(K)]
    state = [bool(down0[0][k]) for k in range(K)]
    nxt = [0] * K
    units = [[0, 0.0, 0, 0.0] for _ in range(K)]
    for n in range(1, years * H + 1):
        for k in range(K):
            while Tl[k][nxt[k]] <= n:
                state[k] = not state[k]
                nxt[k] += 1
        cav = 0.0
        for k in range(K):
            cav += 0.0 if state[k] else cap[k]
        l = L_year[(n - 1) % H]
        if cav < l:
            d = l - cav
            for k in range(K):
                if state[k]:
                    u = units[k]
                    u[0] += 1
                    u[1] += d
                    if not (cav + cap[k] < l):
                        u[2] += 1
                    u[3] += min(d, cap[k])
    return np.array(units, dtype=np.float64)
