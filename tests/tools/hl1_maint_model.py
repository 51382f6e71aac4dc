"""Host model of planned maintenance on the HL1 sequential chronology (relmc_hl1_maint_seq, contract in include/relmc.h).

The chronology is hl1_seq_model's (chronology: start states and transition times from the contract's draws); a schedule is a list of
windows (unit, start_hour, hours) in hours of the year.  Per step the capacity is summed over the units in ascending order, a unit adding
its capacity when it is UP and not on maintenance and 0.0 otherwise; a unit is on maintenance at hour-of-year h when some window of it has
(h - start_hour) mod H < hours.  Loss hours, EUE and loss events per year are taken as hl1_seq_model.interval_chain takes them, and a
schedule without windows is that function's result.  The load is scale * load + shift, numpy rounding the product and the sum as the
contract does.  Nothing here builds a mask table: the window rule is evaluated per unit on the steps' hours.
"""
import importlib.util
import os

import numpy as np

_spec = importlib.util.spec_from_file_location("hl1_seq_model", os.path.join(os.path.dirname(os.path.abspath(__file__)), "hl1_seq_model.py"))
SEQ = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(SEQ)


def on_maintenance(windows, unit: int, hour, H: int) -> np.ndarray:
    """Whether `unit` is on maintenance at the hours-of-year `hour` (array) under the windows (unit, start_hour, hours)."""
    hour = np.asarray(hour, dtype=np.int64)
    on = np.zeros(hour.shape, dtype=bool)
    for k, s, m in windows:
        if k == unit:
            on |= (hour - s) % H < m
    return on


def maint_chain(down0, T, cap, curve, years: int, windows):
    """One chain under one schedule: down0[K], T[K, E] -> per-year arrays (loss hours, EUE, loss events) of length `years`."""
    curve = np.asarray(curve, dtype=np.float64)
    H = curve.size
    S = years * H
    n = np.arange(1, S + 1, dtype=np.float64)
    hour = (np.arange(S, dtype=np.int64)) % H                      # step n is hour (n - 1) mod H
    cav = np.zeros(S)
    for k in range(len(cap)):                                      # ascending unit order, + 0.0 for a unit that does not count (exact)
        cnt = np.searchsorted(T[k], n, side="right")               # #{T_j <= n}
        down = down0[k] ^ (cnt & 1).astype(bool)
        cav = cav + np.where(down | on_maintenance(windows, k, hour, H), 0.0, float(cap[k]))
    ld = np.tile(curve, years)
    loss = cav < ld
    deficit = np.where(loss, ld - cav, 0.0)
    prev = np.concatenate([[False], loss[:-1]])
    rise = loss & ~prev
    return (loss.reshape(years, H).sum(1).astype(np.float64), deficit.reshape(years, H).sum(1),
            rise.reshape(years, H).sum(1).astype(np.float64))


def maint_model(seed: int, chains, cap, mttf, mttr, load, years: int, start: int, schedules, scale: float = 1.0, shift: float = 0.0):
    """schedules: lists of (unit, start_hour, hours) -> arrays [n_schedules, nchains * years] of loss hours, EUE and loss events,
    chain-major.  Every schedule sees the one chronology of a chain."""
    chains = np.atleast_1d(np.asarray(chains, dtype=np.uint64))
    curve = np.float64(scale) * np.asarray(load, dtype=np.float64) + np.float64(shift)
    out = [[[] for _ in range(3)] for _ in schedules]
    for c0 in range(0, chains.size, 256):
        down0, T, _ = SEQ.chronology(seed, chains[c0:c0 + 256], mttf, mttr, start, years * curve.size)
        for c in range(down0.shape[0]):
            for j, windows in enumerate(schedules):
                for q, a in enumerate(maint_chain(down0[c], T[c], cap, curve, years, windows)):
                    out[j][q].append(a)
    return tuple(np.stack([np.concatenate(out[j][q]) for j in range(len(schedules))]) for q in range(3))
