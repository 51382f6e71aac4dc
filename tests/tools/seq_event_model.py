"""Model of relmc_seq_events (include/relmc.h) in plain Python: the loss events of per-hour system curtailments and component masks.

The oracle has no event output.  `oracle_hours` composes its parts as seqMain.m does -- chronology (seq_mcsampling) -> contingency hours ->
hourly OPF (seq_mcsimulation) -> per-hour curtailment -- and `events_model` derives events, masks, accumulators and the duration histogram
from such hours in plain loops with left-to-right sums.  `events_brute` is a second restatement that labels every hour on its own; the CPU
tests hold the two against each other.  tests/test_seq_events_host.py and tests/test_seq_events.py use this file.
"""
from __future__ import annotations

import numpy as np

MAX_COMP = 256
WORDS = MAX_COMP // 32


def pack_words(states, mw: int) -> np.ndarray:
    """states[..., ncomp] (1 = down) -> uint32 words[..., mw], bit k of word k // 32 = component k."""
    st = np.asarray(states) != 0
    out = np.zeros(st.shape[:-1] + (mw,), dtype=np.uint32)
    for k in range(st.shape[-1]):
        out[..., k >> 5] |= st[..., k].astype(np.uint32) << np.uint32(k & 31)
    return out


def _bits(words) -> list[int]:
    return [32 * q + b for q in range(len(words)) for b in range(32) if (int(words[q]) >> b) & 1]


def events_model(curt, words, threshold: float, n_bins: int = 0) -> dict:
    """curt[years][hpy], words[years][hpy][mw] -> dict(events=[dict], acc=dict, hist=int64[n_bins]).

    An event is a maximal run of hours with curt > threshold inside one year; the record fields are relmc_seq_event's (onset / involved as
    lists of WORDS ints).  acc holds relmc_seq_event_acc's fields: the per-component sums run over the events in list order, sum_energy and
    sum_energy2 over the events left to right."""
    curt = np.asarray(curt, dtype=np.float64)
    words = np.asarray(words, dtype=np.uint32)
    years, hpy = curt.shape
    mw = words.shape[2]
    events = []
    for y in range(years):
        h = 0
        while h < hpy:
            if not curt[y, h] > threshold:
                h += 1
                continue
            start = h
            energy, peak = 0.0, -np.inf
            involved = [0] * WORDS
            while h < hpy and curt[y, h] > threshold:
                v = float(curt[y, h])
                energy = energy + v
                peak = max(peak, v)
                for q in range(mw):
                    involved[q] |= int(words[y, h, q])
                h += 1
            onset = [0] * WORDS
            for q in range(mw):
                before = int(words[y, start - 1, q]) if start > 0 else 0
                onset[q] = int(words[y, start, q]) & ~before & 0xFFFFFFFF
            events.append(dict(year=y, start_hour=start, duration=h - start, censored=1 if h == hpy else 0, energy_mwh=energy, peak_mw=peak,
                               onset=onset, involved=involved))
    acc = dict(years=years, events=len(events), censored=0, load_onset_events=0, sum_dur=0, sum_dur2=0, max_dur=0, sum_energy=0.0, sum_energy2=0.0,
               max_energy=0.0, max_peak=0.0, onset_events=[0] * MAX_COMP, involved_events=[0] * MAX_COMP, onset_energy=[0.0] * MAX_COMP,
               involved_energy=[0.0] * MAX_COMP)
    hist = np.zeros(n_bins, dtype=np.int64)
    for e in events:
        d = e["duration"]
        acc["censored"] += e["censored"]
        acc["load_onset_events"] += 0 if any(e["onset"]) else 1
        acc["sum_dur"] += d
        acc["sum_dur2"] += d * d
        acc["max_dur"] = max(acc["max_dur"], d)
        acc["sum_energy"] += e["energy_mwh"]
        acc["sum_energy2"] += e["energy_mwh"] * e["energy_mwh"]
        acc["max_energy"] = max(acc["max_energy"], e["energy_mwh"])
        acc["max_peak"] = max(acc["max_peak"], e["peak_mw"])
        for k in _bits(e["onset"]):
            acc["onset_events"][k] += 1
            acc["onset_energy"][k] += e["energy_mwh"]
        for k in _bits(e["involved"]):
            acc["involved_events"][k] += 1
            acc["involved_energy"][k] += e["energy_mwh"]
        if n_bins:
            hist[min(d, n_bins) - 1] += 1
    return dict(events=events, acc=acc, hist=hist)


def events_brute(curt, states, threshold: float) -> list[tuple]:
    """Second restatement, hour by hour on boolean states[years][hpy][ncomp]: every loss hour is labelled with the first hour of its run
    (the last hour at or before it whose predecessor is not a loss hour), and the runs are collected from the labels.
    Returns [(year, start, duration, censored, energy, peak, onset component tuple, involved component tuple)]."""
    curt = np.asarray(curt, dtype=np.float64)
    st = np.asarray(states) != 0
    years, hpy = curt.shape
    out = []
    for y in range(years):
        flag = [bool(curt[y, h] > threshold) for h in range(hpy)]
        label = {}
        for h in range(hpy):
            if flag[h]:
                s = h
                while s > 0 and flag[s - 1]:
                    s -= 1
                label.setdefault(s, []).append(h)
        for s in sorted(label):
            hrs = label[s]
            energy = 0.0
            for h in hrs:
                energy += float(curt[y, h])
            onset = tuple(int(k) for k in np.flatnonzero(st[y, s] & ~(st[y, s - 1] if s > 0 else np.zeros_like(st[y, s]))))
            involved = tuple(int(k) for k in np.flatnonzero(st[y, hrs].any(axis=0)))
            out.append((y, s, len(hrs), 1 if hrs[-1] == hpy - 1 else 0, energy, max(float(curt[y, h]) for h in hrs), onset, involved))
    return out


def event_tuples(model: dict) -> list[tuple]:
    """events_model's list in events_brute's form."""
    return [(e["year"], e["start_hour"], e["duration"], e["censored"], e["energy_mwh"], e["peak_mw"], tuple(_bits(e["onset"])), tuple(_bits(e["involved"])))
            for e in model["events"]]


def oracle_hours(oracle, rel, hpy: int, load_factors, seed: int, first_year: int, n_years: int, policy=0, nthreads: int = 8) -> dict:
    """seqMain.m:91-141 from the oracle's parts: dict(curt[years][hpy], states[years][hpy][ncomp], n_contingency, status of the contingency hours)."""
    lf = np.asarray(load_factors, dtype=np.float64)
    st = oracle.seq_mcsampling(rel, hpy, seed, first_year, n_years)                    # [years * hpy, ncomp]
    hours = np.flatnonzero(st.sum(1) > 0)                                              # seqMain.m:97
    curt = np.zeros(n_years * hpy)
    status = np.zeros(0, dtype=np.int32)
    if hours.size:
        r = oracle.seq_mcsimulation(st[hours], lf[hours % hpy], policy, nthreads=nthreads)
        curt[hours] = r["dns"]
        status = r["status"]
    return dict(curt=curt.reshape(n_years, hpy), states=st.reshape(n_years, hpy, -1), n_contingency=int(hours.size), status=status, hours=hours)


def oracle_events(oracle, rel, hpy: int, load_factors, seed: int, first_year: int, n_years: int, threshold: float, mw: int, n_bins: int = 0, policy=0) -> dict:
    """events_model on oracle_hours; the hours ride along under "hours"."""
    hrs = oracle_hours(oracle, rel, hpy, load_factors, seed, first_year, n_years, policy)
    m = events_model(hrs["curt"], pack_words(hrs["states"], mw), threshold, n_bins)
    m["hours"] = hrs
    return m
