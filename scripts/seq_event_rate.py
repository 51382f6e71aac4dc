"""Loss events of the sequential HL2 track (relmc_seq_events) beside the step they stand behind: 64 natural RTS-24 years (8736 hours each)
in one call.  Three forms, alternated in one process on the same years, 5 rounds after a warm-up round:
  years        relmc_seq_years
  events       relmc_seq_events, histogram, no list
  events+list  the same with a list that holds every event
Prints relmc_last_kernel_ms (median, min, max) of each form, the ratios events / years of the medians, the run-to-run spread of
relmc_seq_years itself ((max - min) / median over its five repeats) to hold the ratios against, the event count and the code-object hash.
  python scripts/seq_event_rate.py [--years N] [--seed S]"""
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from powersystemsreliabilityassessment_amd import _lib, api, case24, seq  # noqa: E402


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


if __name__ == "__main__":
    years, seed = int(arg("--years", "64")), int(arg("--seed", "1"))
    eng = api.Engine(case24.rts24(), device=0)
    se = seq.SeqEngine(eng)
    last = {}

    def run_years():
        last["years"] = se.seq_years(seed, 0, years)
        return eng.last_kernel_ms()

    def run_events(cap):
        last["events"] = se.seq_events(seed, 0, years, events_cap=cap)
        return eng.last_kernel_ms()

    forms = {"years": run_years, "events": lambda: run_events(0), "events+list": lambda: run_events(years * 4368)}
    ms = {k: [] for k in forms}
    for r in range(6):                                   # round 0 warms up: code objects, buffers
        for k, fn in forms.items():
            m = fn()
            if r:
                ms[k].append(m)
        ev = last["events"]
        assert np.array_equal(ev.nlc, last["years"][2]) and ev.n_events == int(ev.nlc.sum()) and ev.ev_acc.sum_dur == int(ev.dlc.sum()), "the two entries disagree"
    med = {k: statistics.median(v) for k, v in ms.items()}
    for k in forms:
        print(f"{k:12s} relmc_last_kernel_ms median {med[k]:9.3f} min {min(ms[k]):9.3f} max {max(ms[k]):9.3f}", flush=True)
    spread = (max(ms["years"]) - min(ms["years"])) / med["years"]
    print(f"events / years {med['events'] / med['years']:.4f}   events+list / years {med['events+list'] / med['years']:.4f}   "
          f"run-to-run spread of years (max - min) / median {spread:.4f}")
    ev = last["events"]
    print(f"{years} years from seed {seed}: {int(ev.n_contingency.sum())} hourly OPFs, {ev.n_events} events, LOLF {ev.lolf:.4f} occ/yr, "
          f"{ev.mean_duration:.3f} hr/occ, longest {ev.max_duration} h, {ev.ev_acc.load_onset_events} without a new outage")
    print(f"code object {_lib.code_object_sha256()[:12]}")
    eng.close()
