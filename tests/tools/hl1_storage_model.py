"""Host model of energy storage on the HL1 sequential chronology (relmc_hl1_seq_storage, contract in include/relmc.h).

The fleet history is the sequential model's (hl1_seq_model.chronology: same draws, same start rules); cap_avail repeats
interval_chain's ascending loop over the units.  The step loop is the contract's, written in plain Python floats: every operation is one
correctly rounded fp64 operation.  A storage is a tuple (charge_mw, discharge_mw, energy_mwh, eta_charge, eta_discharge, soc0_mwh).

Besides the year records the model counts how often each path of the step loop ran, so that a test can show its fixtures reach them,
and how many 64-step groups of a chain are not quiet (a lane short, or a storage that can charge and is not full at the group's first
step): the groups that take the device kernel's serial stage.

literal_storage_chain restates the contract without any of that: the reference's hour loop for the units (hl1_seq_model.literal_chain's)
with the storages inside it, sharing only the draws with storage_model.  tests/test_hl1_chrono_edges_host.py holds the two against each
other, and both against lane_edge_pattern, a second pattern worked out by hand whose short steps sit at the device's lane and group edges.
"""
import importlib.util
import os

import numpy as np

_spec = importlib.util.spec_from_file_location("hl1_seq_model", os.path.join(os.path.dirname(os.path.abspath(__file__)), "hl1_seq_model.py"))
SEQ = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(SEQ)

WINDOW = 512      # HL1_SEQ_WINDOW: the device's groups are 64 steps of a 512-step window (the chain's last window may end in a short group)


def cap_avail(down0, T, cap, nsteps: int) -> np.ndarray:
    """cap_avail of steps 1 .. nsteps of one chain, interval_chain's sum: ascending unit order, + 0.0 for a DOWN unit (exact)."""
    n = np.arange(1, nsteps + 1, dtype=np.float64)
    cav = np.zeros(nsteps)
    for k in range(len(cap)):
        cnt = np.searchsorted(T[k], n, side="right")               # #{T_j <= n}
        down = down0[k] ^ (cnt & 1).astype(bool)
        cav = cav + np.where(down, 0.0, float(cap[k]))
    return cav


def level_curve(load, scale: float, shift: float) -> np.ndarray:
    """L(h) = scale * load[h] + shift, each operation rounded once."""
    return np.float64(scale) * np.asarray(load, dtype=np.float64) + np.float64(shift)


def new_counters() -> dict:
    return dict(short=0, long=0, equal=0, served=0, lost=0, clamp=0, full_clamp=0, groups=0, serial_groups=0,
                discharge=[0] * 8, charge=[0] * 8, empty_after=[0] * 8)


def storage_chain(cav, curve, years: int, storages, counters=None, trace=None):
    """One chain: cav[S] and the level's curve[H] -> rec[years, 6] = per year lole, eue, lolf, served, discharged, charged, and the final
    states of charge.  trace: an optional list that receives (states of charge after the step, deficit of the step) per step."""
    H = len(curve)
    S = years * H
    cnt = counters if counters is not None else new_counters()
    st = [tuple(float(v) for v in s) for s in storages]
    soc = [s[5] for s in st]
    cav = [float(v) for v in cav]
    curve = [float(v) for v in curve]
    rec = np.zeros((years, 6))
    prev = False
    for n in range(S):
        y, h = divmod(n, H)
        if n % WINDOW % 64 == 0:                                   # first step of a device group
            cnt["groups"] += 1
            g1 = min(n + 64, S)
            if any(cav[q] < curve[q % H] for q in range(n, g1)) or any(soc[i] < s[2] and s[0] > 0.0 for i, s in enumerate(st)):
                cnt["serial_groups"] += 1
        cap, L = cav[n], curve[h]
        loss = False
        need = 0.0
        if cap < L:
            cnt["short"] += 1
            need = L - cap
            xs = 0.0
            for i, (chg, dis, en, ec, ed, _) in enumerate(st):
                if not need > 0.0:
                    break
                avail = min(dis, soc[i] * ed)
                x = min(avail, need)
                t = soc[i] - x / ed
                if t < 0.0:
                    cnt["clamp"] += 1
                soc[i] = max(0.0, t)
                need = need - x
                xs = xs + x
                if x > 0.0:
                    cnt["discharge"][i] += 1
            rec[y, 4] += xs
            if need > 0.0:
                loss = True
                cnt["lost"] += 1
                rec[y, 0] += 1.0
                rec[y, 1] += need
                if not prev:
                    rec[y, 2] += 1.0
            else:
                cnt["served"] += 1
                rec[y, 3] += 1.0
        elif cap > L:
            cnt["long"] += 1
            surplus = cap - L
            ys = 0.0
            for i, (chg, dis, en, ec, ed, _) in enumerate(st):
                if not surplus > 0.0:
                    break
                room = (en - soc[i]) / ec
                yv = min(min(chg, room), surplus)
                t = soc[i] + yv * ec
                if t > en:
                    cnt["full_clamp"] += 1
                soc[i] = min(en, t)
                surplus = surplus - yv
                ys = ys + yv
                if yv > 0.0:
                    cnt["charge"][i] += 1
            rec[y, 5] += ys
        else:
            cnt["equal"] += 1
        for i in range(len(st)):
            if soc[i] == 0.0:
                cnt["empty_after"][i] += 1
        if trace is not None:
            trace.append((tuple(soc), need if loss else 0.0))
        prev = loss
    return rec, soc


def hand_pattern():
    """One 100 MW unit that never fails, a ten-hour year and one storage of 20 MW / 30 MWh with efficiencies 1.0 (charge) and 0.5
    (discharge), started full: every number is dyadic, so every sum is exact in any order.  Two years, the second starting empty inside
    a loss event.  -> (curve, storage, soc after each of the 20 steps, deficit of each step, rec[2, 6]); tests/test_hl1_storage_host.py
    derives the numbers step by step."""
    curve = [103.0, 110.0, 112.0, 104.0, 100.0, 96.0, 101.0, 60.0, 50.0, 130.0]
    storage = (20.0, 20.0, 30.0, 1.0, 0.5, 30.0)
    soc = [24.0, 4.0, 0.0, 0.0, 0.0, 4.0, 2.0, 22.0, 30.0, 0.0,
           0.0, 0.0, 0.0, 0.0, 0.0, 4.0, 2.0, 22.0, 30.0, 0.0]
    deficit = [0.0, 0.0, 10.0, 4.0, 0.0, 0.0, 0.0, 0.0, 0.0, 15.0,
               3.0, 10.0, 12.0, 4.0, 0.0, 0.0, 0.0, 0.0, 0.0, 15.0]
    rec = np.array([[3.0, 29.0, 2.0, 3.0, 31.0, 32.0],
                    [5.0, 44.0, 1.0, 1.0, 16.0, 32.0]])
    return curve, storage, soc, deficit, rec


def lane_edge_pattern():
    """One 100 MW unit that never fails, a 130-hour year (two 64-step groups and two steps: the year's place in the device's groups moves
    by two lanes a year) and one storage of 3 MW charge / 16 MW discharge / 32 MWh with efficiencies 1.0 (charge) and 0.5 (discharge),
    started full: every number is dyadic, so every sum is exact in any order.  The load is 96 MW (a surplus of 4) except on the 0-based
    hours 62, 63, 64 (needs 4, 16, 8) and 127, 128, 129 (needs 6, 12, 2).  Three years: 390 steps, so the chain's last group has six steps.

    0-based steps of the short hours -> lane of their 64-step group (step mod 64):
      year 1: 62, 63, 64 -> lanes 62, 63 | 0 (the run crosses a group edge);  127, 128, 129 -> lanes 63 | 0, 1; the year ends at lane 1
      year 2: 192, 193, 194 -> lanes 0, 1, 2;  257, 258, 259 -> lanes 1, 2, 3
      year 3: 322, 323, 324 -> lanes 2, 3, 4;  387, 388, 389 -> lanes 3, 4, 5 of the six-step last group; step 389 ends the chain
    Every year (s = state of charge; a delivered MW costs 2 MWh):
      hour 62   need 4:  avail min(16, 32 * .5) = 16, x 4,  s 32 - 8  = 24             served
      hour 63   need 16: avail min(16, 12) = 12,      x 12, s 24 - 24 = 0, deficit 4   the storage runs empty inside the run: event 1
      hour 64   need 8:  avail 0                                           deficit 8   still event 1
      65 - 126  surplus 4: y = min(3, room, 4) = 3 for ten hours (s 30), then room 2: y 2 (s 32, exactly full), then y 0: charged 32
      hour 127  need 6:  avail 16,                    x 6,  s 32 - 12 = 20             served
      hour 128  need 12: avail min(16, 10) = 10,      x 10, s 20 - 20 = 0, deficit 2   event 2
      hour 129  need 2:  avail 0                                           deficit 2   still event 2; the year ends empty
      per year  lole 4, eue 4 + 8 + 2 + 2 = 16, lolf 2, served 2, discharged 4 + 12 + 6 + 10 = 32
    Hours 0 - 61: full in year 1 (nothing charged: 32 in the year); empty in years 2 and 3, filled as in hours 65 - 126 (64 in the year).
    -> (curve, storage, years, rec[3, 6])."""
    curve = [96.0] * 130
    for h, need in ((62, 4.0), (63, 16.0), (64, 8.0), (127, 6.0), (128, 12.0), (129, 2.0)):
        curve[h] = 100.0 + need
    storage = (3.0, 16.0, 32.0, 1.0, 0.5, 32.0)
    rec = np.array([[4.0, 16.0, 2.0, 2.0, 32.0, 32.0],
                    [4.0, 16.0, 2.0, 2.0, 32.0, 64.0],
                    [4.0, 16.0, 2.0, 2.0, 32.0, 64.0]])
    return curve, storage, 3, rec


def literal_storage_chain(seed: int, chain: int, cap, mttf, mttr, load, years: int, start: int, storages, scale: float = 1.0,
                          shift: float = 0.0, counters=None) -> np.ndarray:
    """The contract of relmc_hl1_seq_storage (include/relmc.h) as one plain loop, in Python floats: hours outside, units and then
    storages inside; no groups, lanes, bits or skipped steps.  The unit states are hl1_seq_model.literal_chain's hour loop (`ttf -= 1;
    while ttf <= 0: toggle, ttf += duration`, the reference's), so the capacity side does not come from the interval form either; only
    the draws (SEQ.chronology's U) are shared.  Nothing of storage_chain is used.  -> rec[years, 6] = per year lole, eue, lolf,
    served_hours, discharged_mwh, charged_mwh, each summed over the year's hours in hour order.  counters: an optional dict that
    receives how often the steps were short / long / served / lost and how often storage i delivered or took energy."""
    K, H = len(cap), len(load)
    _, _, U = SEQ.chronology(seed, [chain], mttf, mttr, start, years * H)
    u, lnU = U[0].tolist(), np.log(U[0]).tolist()
    mttf, mttr, cap, load = ([float(x) for x in v] for v in (mttf, mttr, cap, load))
    scale, shift = float(scale), float(shift)
    status, ttf, ev = [True] * K, [0.0] * K, [0] * K
    for i in range(K):
        if start == SEQ.STATIONARY:
            status[i] = not (u[i][0] < mttr[i] / (mttf[i] + mttr[i]))
            ev[i] = 1
        ttf[i] = -(mttf[i] if status[i] else mttr[i]) * lnU[i][ev[i]]
        ev[i] += 1
    P = [dict(zip(("charge", "discharge", "energy", "eta_c", "eta_d"), (float(v) for v in s[:5]))) for s in storages]
    soc = [float(s[5]) for s in storages]
    cnt = counters if counters is not None else {}
    for key in ("short", "long", "served", "lost"):
        cnt.setdefault(key, 0)
    cnt.setdefault("discharge", [0] * 8)
    cnt.setdefault("charge", [0] * 8)
    rec = np.zeros((years, 6))
    was_loss = False
    for y in range(years):
        lole = eue = lolf = served = discharged = charged = 0.0
        for h in range(H):
            cap_avail = 0.0
            for i in range(K):
                ttf[i] -= 1.0
                while ttf[i] <= 0:
                    status[i] = not status[i]
                    ttf[i] += -(mttf[i] if status[i] else mttr[i]) * lnU[i][ev[i]]
                    ev[i] += 1
                if status[i]:
                    cap_avail += cap[i]
            product = scale * load[h]
            L = product + shift
            loss = False
            if cap_avail < L:
                cnt["short"] += 1
                need = L - cap_avail
                delivered = 0.0
                for i, p in enumerate(P):
                    if not need > 0.0:
                        break
                    avail = min(p["discharge"], soc[i] * p["eta_d"])
                    x = min(avail, need)
                    soc[i] = max(0.0, soc[i] - x / p["eta_d"])
                    need = need - x
                    delivered = delivered + x
                    cnt["discharge"][i] += x > 0.0
                discharged += delivered
                if need > 0.0:
                    loss = True
                    cnt["lost"] += 1
                    lole += 1.0
                    eue += need
                    if not was_loss:
                        lolf += 1.0
                else:
                    cnt["served"] += 1
                    served += 1.0
            elif cap_avail > L:
                cnt["long"] += 1
                surplus = cap_avail - L
                taken = 0.0
                for i, p in enumerate(P):
                    if not surplus > 0.0:
                        break
                    room = (p["energy"] - soc[i]) / p["eta_c"]
                    yv = min(min(p["charge"], room), surplus)
                    soc[i] = min(p["energy"], soc[i] + yv * p["eta_c"])
                    surplus = surplus - yv
                    taken = taken + yv
                    cnt["charge"][i] += yv > 0.0
                charged += taken
            was_loss = loss
        rec[y] = (lole, eue, lolf, served, discharged, charged)
    return rec


def storage_model(seed: int, chains, cap, mttf, mttr, load, years: int, start: int, storages, scale: float = 1.0, shift: float = 0.0,
                  counters=None):
    """Chains `chains` -> (rec[nchains * years, 6], counters): per year lole, eue, lolf, served_hours, discharged_mwh, charged_mwh,
    chain-major.  EUE and the two energies are summed over a year's steps in step order (the device sums lane partials; the tests
    compare them to a relative tolerance)."""
    chains = np.atleast_1d(np.asarray(chains, dtype=np.uint64))
    curve = level_curve(load, scale, shift)
    H = curve.size
    cnt = counters if counters is not None else new_counters()
    out = []
    for c0 in range(0, chains.size, 256):
        down0, T, _ = SEQ.chronology(seed, chains[c0:c0 + 256], mttf, mttr, start, years * H)
        for c in range(down0.shape[0]):
            rec, _ = storage_chain(cap_avail(down0[c], T[c], cap, years * H), curve, years, storages, cnt)
            out.append(rec)
    return np.concatenate(out), cnt
