"""Host model of the loss events of the HL1 sequential chronology (relmc_hl1_seq_events, include/relmc.h).

A loss event of a chain is a maximal run of consecutive loss steps among its steps 1 .. Y*H: start step n0 (1-based), duration D,
energy E (the deficits summed in ascending step order), peak P (the largest deficit), censored iff the run reaches step Y*H.

  (a) interval_events: the loss / deficit arrays of hl1_seq_model's interval form (its `chronology`, imported, not changed),
      run-length encoded.
  (b) literal_events: the reference's hour loop (hl1_seq_model.literal_chain's transliteration of PowerSystemAdequacy.jl:214-268) with the
      event bookkeeping done inside the loop, hour by hour.
  (c) pattern cases: a load curve that is +1e9 on chosen hours and -1.0 elsewhere makes the loss flag independent of every draw
      (0 <= cap_avail < 1e9: never a loss at a negative load, always one at 1e9), so the event list can be written out by hand.
"""
from __future__ import annotations

import importlib.util
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("hl1_seq_model", os.path.join(_HERE, "hl1_seq_model.py"))
SEQ = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(SEQ)

ALL_UP, STATIONARY = SEQ.ALL_UP, SEQ.STATIONARY
EVENT = np.dtype([("chain", np.int64), ("start_step", np.int64), ("duration", np.int64), ("energy_mwh", np.float64), ("peak_mw", np.float64)])
PATTERN_HIGH, PATTERN_LOW = 1e9, -1.0


def rle(loss, deficit, chain: int = 0) -> np.ndarray:
    """Events of one chain from its per-step loss flags and deficits (index 0 = step 1)."""
    loss = np.asarray(loss, dtype=bool)
    edge = np.diff(np.concatenate([[0], loss.astype(np.int8), [0]]))
    first, past = np.flatnonzero(edge == 1), np.flatnonzero(edge == -1)      # 0-based first step, one past the last
    ev = np.zeros(first.size, dtype=EVENT)
    ev["chain"], ev["start_step"], ev["duration"] = chain, first + 1, past - first
    for j, (a, b) in enumerate(zip(first, past)):
        e = 0.0
        for x in deficit[a:b].tolist():                                       # ascending step order
            e += x
        ev["energy_mwh"][j], ev["peak_mw"][j] = e, deficit[a:b].max()
    return ev


def loss_arrays(down0, T, cap, load, years: int):
    """One chain of the interval form: per-step loss flag and deficit (cap_avail over the UP units in ascending order)."""
    load = np.asarray(load, dtype=np.float64)
    S = years * load.size
    n = np.arange(1, S + 1, dtype=np.float64)
    cav = np.zeros(S)
    for k in range(len(cap)):
        cnt = np.searchsorted(T[k], n, side="right")
        down = down0[k] ^ (cnt & 1).astype(bool)
        cav = cav + np.where(down, 0.0, float(cap[k]))
    ld = np.tile(load, years)
    loss = cav < ld
    return loss, np.where(loss, ld - cav, 0.0)


def interval_events(seed: int, chains, cap, mttf, mttr, load, years: int, start: int, first_chain: int | None = None) -> np.ndarray:
    """(a) for chains `chains`: every event in (chain, start_step) order, `chain` relative to first_chain (default chains[0])."""
    chains = [int(c) for c in chains]
    base = chains[0] if first_chain is None else first_chain
    H = np.asarray(load).size
    out = []
    for c0 in range(0, len(chains), 256):
        down0, T, _ = SEQ.chronology(seed, chains[c0:c0 + 256], mttf, mttr, start, years * H)
        for j in range(down0.shape[0]):
            loss, deficit = loss_arrays(down0[j], T[j], cap, load, years)
            out.append(rle(loss, deficit, chains[c0 + j] - base))
    return np.concatenate(out) if out else np.zeros(0, dtype=EVENT)


def literal_events(seed: int, chain: int, cap, mttf, mttr, load, years: int, start: int, rel_chain: int = 0) -> np.ndarray:
    """(b) one chain by the reference's hour loop; an event is opened at a rising loss flag and extended hour by hour."""
    K, H = len(cap), len(load)
    _, _, U = SEQ.chronology(seed, [chain], mttf, mttr, start, years * H)
    u, lnU = U[0].tolist(), np.log(U[0]).tolist()
    mttf, mttr, cap, load = ([float(x) for x in v] for v in (mttf, mttr, cap, load))
    status, ttf, ev = [True] * K, [0.0] * K, [0] * K
    for i in range(K):
        if start == STATIONARY:
            status[i] = not (u[i][0] < mttr[i] / (mttf[i] + mttr[i]))
            ev[i] = 1
        ttf[i] = -(mttf[i] if status[i] else mttr[i]) * lnU[i][ev[i]]
        ev[i] += 1
    events, cur, n = [], None, 0
    for _y in range(years):
        for h in range(H):
            n += 1
            cap_avail = 0.0
            for i in range(K):
                ttf[i] -= 1.0
                while ttf[i] <= 0:
                    status[i] = not status[i]
                    ttf[i] += -(mttf[i] if status[i] else mttr[i]) * lnU[i][ev[i]]
                    ev[i] += 1
                if status[i]:
                    cap_avail += cap[i]
            if cap_avail < load[h]:
                d = load[h] - cap_avail
                if cur is None:
                    cur = [rel_chain, n, 0, 0.0, 0.0]
                cur[2] += 1; cur[3] += d; cur[4] = max(cur[4], d)
            elif cur is not None:
                events.append(tuple(cur)); cur = None
    if cur is not None:
        events.append(tuple(cur))
    return np.array(events, dtype=EVENT)


def kinds(ev: np.ndarray, H: int, years: int) -> dict:
    """How many events of each edge kind a list holds: D = 1, crossing a 64-step group edge / a 512-step window edge / a year boundary
    (steps n and n + 1 of the event with n a multiple of 64 / 512 / H), starting at step 1, censored (reaching step years * H)."""
    a, b = ev["start_step"], ev["start_step"] + ev["duration"] - 1              # first and last step
    cross = lambda m: int(np.sum(((b - 1) // m) * m >= a))                      # a multiple n of m with a <= n < b
    return {"n": int(ev.size), "d1": int(np.sum(ev["duration"] == 1)), "edge64": cross(64), "edge512": cross(512), "year": cross(H),
            "step1": int(np.sum(a == 1)), "censored": int(np.sum(b == years * H))}


def summary(ev: np.ndarray, H: int, years: int, n_bins: int):
    """relmc_hl1_event_acc's fields (without `years`) and the duration histogram of an event list."""
    D, E = ev["duration"], ev["energy_mwh"]
    hist = np.bincount(np.minimum(D, n_bins) - 1, minlength=n_bins).astype(np.int64) if ev.size else np.zeros(n_bins, dtype=np.int64)
    end = ev["start_step"] + D - 1
    acc = {"events": int(ev.size), "censored": int(np.sum(end == years * H)), "sum_dur": int(D.sum()), "sum_dur2": int((D * D).sum()),
           "max_dur": int(D.max(initial=0)), "sum_energy": float(E.sum()), "sum_energy2": float((E * E).sum()),
           "max_energy": float(E.max(initial=0.0)), "max_peak": float(ev["peak_mw"].max(initial=0.0))}
    return acc, hist


# ---- (c) deterministic patterns --------------------------------------------------------------------------------------------------
def pattern_load(nhours: int, loss_hours) -> np.ndarray:
    """Load curve of one year with a certain loss on the 0-based hours `loss_hours` and certainly none elsewhere."""
    load = np.full(nhours, PATTERN_LOW)
    load[list(loss_hours)] = PATTERN_HIGH
    return load


def pattern_unit():
    """One 100 MW unit (any rates do: the loss flag does not depend on its state; the deficit does: 1e9 - 100 when UP, 1e9 when DOWN)."""
    return np.array([100.0]), np.array([900.0]), np.array([100.0])
