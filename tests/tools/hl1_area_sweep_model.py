"""Host model of the multi-area sweep (relmc_hl1_area_sweep, include/relmc.h): a level IS the model it is equivalent to, so the model of
a sweep is a loop of hl1_area_model.interval_model (hl1_tie_model.interval_model with tie outage data) over the transformed systems:

  load   of area a: scale[a] * load[a] + shift[a] (numpy: the product and the sum each rounded)
  ties   capacity tie_scale * cap_t where the tie is scaled (tie_scaled None, or tie_scaled[t]), else cap_t
  fleet  1: the withheld units' capacities as 0.0 (they keep their global indices, hence their draws)

A level is (scale, shift, tie_scale, fleet) with scale / shift scalars or one value per area.
"""
from __future__ import annotations

import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
_spec = importlib.util.spec_from_file_location("hl1_tie_model", os.path.join(ROOT, "tests", "tools", "hl1_tie_model.py"))
TM = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(TM)
AM = TM.AM

ALL_UP, STATIONARY = AM.ALL_UP, AM.STATIONARY
ISOLATED, INTERCONNECTED = AM.ISOLATED, AM.INTERCONNECTED
REFERENCE, MAX_FLOW = AM.REFERENCE, AM.MAX_FLOW


def transform(cap, loads, ties, level, withheld=(), tie_scaled=None):
    """(cap, loads, ties) of the model one level is equivalent to.  ties: 0-based (from, to, capacity)."""
    scale, shift, tie_scale, fleet = level
    loads = np.atleast_2d(np.asarray(loads, dtype=np.float64))
    n = loads.shape[0]
    scale = np.broadcast_to(np.asarray(scale, dtype=np.float64), (n,))
    shift = np.broadcast_to(np.asarray(shift, dtype=np.float64), (n,))
    cap = np.array(cap, dtype=np.float64)
    if fleet:
        cap[list(withheld)] = 0.0
    out = [(i, j, float(tie_scale) * float(c) if tie_scaled is None or tie_scaled[t] else float(c)) for t, (i, j, c) in enumerate(ties)]
    return cap, scale[:, None] * loads + shift[:, None], out


def sweep_model(seed, chains, units_per_area, cap, mttf, mttr, loads, ties, tie_mttf, tie_mttr, years, start, flow, levels, withheld=(),
                tie_scaled=None):
    """[n_levels, len(chains) * years, n + 1, 3]: every level through the interval model of its transformed system, INTERCONNECTED.
    tie_mttf None: no outage data."""
    n = np.atleast_2d(np.asarray(loads)).shape[0]
    out = []
    for level in levels:
        c, ld, tl = transform(cap, loads, ties, level, withheld, tie_scaled)
        if tie_mttf is None:
            out.append(AM.interval_model(seed, chains, units_per_area, c, mttf, mttr, ld, AM.topology(n, tl), years, start, INTERCONNECTED, flow))
        else:
            out.append(TM.interval_model(seed, chains, units_per_area, c, mttf, mttr, ld, tl, tie_mttf, tie_mttr, years, start, INTERCONNECTED, flow))
    return np.stack(out)
