"""Host model of the load sweep on the HL1 sequential chronology (relmc_hl1_seq_sweep, contract in include/relmc.h).

A level (scale, shift, fleet) of a sweep is the sequential model itself (hl1_seq_model.interval_model) on the load curve
scale * load + shift -- numpy rounds the product and the sum as the contract does -- with the capacities of the withheld units set to
0.0 when the level's fleet is 1: the unit's history is still drawn (every level sees the same fleet history), it only adds nothing.
"""
import importlib.util
import os

import numpy as np

_spec = importlib.util.spec_from_file_location("hl1_seq_model", os.path.join(os.path.dirname(os.path.abspath(__file__)), "hl1_seq_model.py"))
SEQ = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(SEQ)


def level_curve(load, scale: float, shift: float) -> np.ndarray:
    """L_j(h) = scale * load[h] + shift, each operation rounded once."""
    return np.float64(scale) * np.asarray(load, dtype=np.float64) + np.float64(shift)


def level_capacities(cap, fleet: int, withheld) -> np.ndarray:
    """The capacities a level sees: those of fleet 1 have 0.0 at the withheld units."""
    c = np.array(cap, dtype=np.float64)
    if fleet == 1:
        c[list(withheld)] = 0.0
    return c


def sweep_model(seed: int, chains, cap, mttf, mttr, load, years: int, start: int, levels, withheld=()):
    """levels: (scale, shift, fleet) triples -> arrays [n_levels, nchains * years] of loss hours, EUE and loss events, chain-major."""
    out = [SEQ.interval_model(seed, chains, level_capacities(cap, fleet, withheld), mttf, mttr, level_curve(load, scale, shift), years, start)
           for scale, shift, fleet in levels]
    return tuple(np.stack([o[q] for o in out]) for q in range(3))
