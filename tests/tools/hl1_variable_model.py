"""Host model of weather-year wind and solar resources on the HL1 sequential chronology (relmc_hl1_var_seq, contract in include/relmc.h).

The fleet history is the sequential model's (hl1_seq_model.chronology: same draws, same start rules) and cap_avail is
hl1_storage_model.cap_avail's ascending loop over the units.  Every chain year draws a weather year w (weather_years: the contract's two
rules, the RANDOM one on oracle.pyoracle.philox4x32_10); a step's capacity is cap_avail plus resource_scale[r] * output[w][r][h] for r
ascending and its load scale * base(w, h) + shift, each operation rounded once.  The step loop over the storages is
hl1_storage_model.storage_chain's, repeated here for a per-step capacity and a per-step load (variable_chain), in plain Python floats,
with the same counters.

literal_variable_chain restates the contract as one plain hour loop (units, then resources, then storages inside it), sharing only the
draws with variable_model.  tests/test_hl1_variable_host.py holds the two against each other and against a pattern worked out by hand.
"""
import importlib.util
import os

import numpy as np

_spec = importlib.util.spec_from_file_location("hl1_storage_model", os.path.join(os.path.dirname(os.path.abspath(__file__)), "hl1_storage_model.py"))
SM = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(SM)
SEQ = SM.SEQ

from oracle.pyoracle import philox4x32_10  # noqa: E402  (hl1_seq_model put the repository root on sys.path)

VAR_TAG = 0x60000000          # RELMC_HL1_VAR_TAG
PICK_RANDOM, PICK_CYCLE = 0, 1
WINDOW = SM.WINDOW
_M64 = (1 << 64) - 1


def weather_year(seed: int, chain: int, y: int, years: int, n_weather: int, pick: int) -> int:
    """The weather year of chain year y (0-based) of `chain`, in Python integers."""
    seed, chain = int(seed), int(chain)
    if pick == PICK_CYCLE:
        return ((chain * years & _M64) + y & _M64) % n_weather
    ctr = np.array([chain & 0xFFFFFFFF, chain >> 32, VAR_TAG, y], dtype=np.uint32)
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint32)
    x = int(philox4x32_10(ctr[None, :], key[None, :])[0, 0])
    return (x * n_weather) >> 32


def weather_years(seed: int, chains, years: int, n_weather: int, pick: int) -> np.ndarray:
    """w[nchains, years] for the chains `chains` (RANDOM in one vectorised Philox call)."""
    ch = [int(c) for c in np.atleast_1d(np.asarray(chains, dtype=np.uint64))]
    if pick == PICK_CYCLE:
        return np.array([[weather_year(seed, c, y, years, n_weather, pick) for y in range(years)] for c in ch], dtype=np.int64).reshape(len(ch), years)
    ctr = np.zeros((len(ch), years, 4), dtype=np.uint32)
    ctr[..., 0] = np.array([c & 0xFFFFFFFF for c in ch], dtype=np.uint32)[:, None]
    ctr[..., 1] = np.array([c >> 32 for c in ch], dtype=np.uint32)[:, None]
    ctr[..., 2] = VAR_TAG
    ctr[..., 3] = np.arange(years, dtype=np.uint32)[None, :]
    key = np.zeros((len(ch), years, 2), dtype=np.uint32)
    key[..., 0] = int(seed) & 0xFFFFFFFF
    key[..., 1] = int(seed) >> 32
    x = philox4x32_10(ctr, key)[..., 0].astype(np.uint64)
    return ((x * np.uint64(n_weather)) >> np.uint64(32)).astype(np.int64)


def step_curves(cav, w, load, weather_out, weather_load, resource_scale, scale: float, shift: float):
    """cap[S] and L[S] of one chain: cav[S] the fleet's cap_avail, w[years] its weather years.  Each operation is one rounded fp64
    operation: cap = cap + scale_r * out[w][r][h] for r ascending, L = scale * base + shift."""
    out = np.asarray(weather_out, dtype=np.float64)
    nw, nres, H = out.shape
    w = np.asarray(w, dtype=np.int64)
    cap = np.asarray(cav, dtype=np.float64).copy()
    for r in range(nres):
        prod = np.float64(resource_scale[r]) * out[w, r, :].reshape(-1)
        cap = cap + prod
    base = np.asarray(weather_load, dtype=np.float64)[w, :].reshape(-1) if weather_load is not None else np.tile(np.asarray(load, dtype=np.float64), w.size)
    prod = np.float64(scale) * base
    return cap, prod + np.float64(shift)


def variable_chain(cap, L, H: int, years: int, storages, counters=None, trace=None):
    """hl1_storage_model.storage_chain for a per-step capacity cap[S] and a per-step load L[S], S = years * H: rec[years, 6] = per year lole,
    eue, lolf, served, discharged, charged, and the final states of charge.  trace: an optional list that receives (states of charge
    after the step, deficit of the step) per step."""
    S = years * H
    cnt = counters if counters is not None else SM.new_counters()
    st = [tuple(float(v) for v in s) for s in storages]
    soc = [s[5] for s in st]
    cap = [float(v) for v in cap]
    L = [float(v) for v in L]
    rec = np.zeros((years, 6))
    prev = False
    for n in range(S):
        y = n // H
        if n % WINDOW % 64 == 0:                                   # first step of a device group
            cnt["groups"] += 1
            g1 = min(n + 64, S)
            if any(cap[q] < L[q] for q in range(n, g1)) or any(soc[i] < s[2] and s[0] > 0.0 for i, s in enumerate(st)):
                cnt["serial_groups"] += 1
        c, l = cap[n], L[n]
        loss = False
        need = 0.0
        if c < l:
            cnt["short"] += 1
            need = l - c
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
        elif c > l:
            cnt["long"] += 1
            surplus = c - l
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
        if trace is not None:
            trace.append((tuple(soc), need if loss else 0.0))
        prev = loss
    return rec, soc


def variable_model(seed: int, chains, cap, mttf, mttr, load, years: int, start: int, weather_out, weather_load=None, resource_scale=None,
                   pick: int = PICK_RANDOM, storages=(), scale: float = 1.0, shift: float = 0.0, counters=None, weather=None):
    """Chains `chains` -> (rec[nchains * years, 6], weather[nchains * years]): per year lole, eue, lolf, served_hours, discharged_mwh,
    charged_mwh and the weather year, chain-major.  weather_out[n_weather, n_resources, H]; weather_load None or [n_weather, H];
    resource_scale None (every resource at 1.0) or one scale per resource.  The energies are summed over a year's steps in step order
    (the device sums lane partials; the tests compare them to a relative tolerance).  counters: as hl1_storage_model's.  weather: None, or
    the weather years [nchains, years] to use in place of the contract's pick (the tests' perturbed models)."""
    chains = np.atleast_1d(np.asarray(chains, dtype=np.uint64))
    out = np.asarray(weather_out, dtype=np.float64)
    nw, nres, H = out.shape
    rs = [1.0] * nres if resource_scale is None else [float(v) for v in resource_scale][:nres]
    cnt = counters if counters is not None else SM.new_counters()
    W = weather_years(seed, chains, years, nw, pick) if weather is None else np.asarray(weather, dtype=np.int64).reshape(chains.size, years)
    recs = []
    for c0 in range(0, chains.size, 256):
        down0, T, _ = SEQ.chronology(seed, chains[c0:c0 + 256], mttf, mttr, start, years * H)
        for c in range(down0.shape[0]):
            cav = SM.cap_avail(down0[c], T[c], cap, years * H)
            cs, Ls = step_curves(cav, W[c0 + c], load, out, weather_load, rs, scale, shift)
            recs.append(variable_chain(cs, Ls, H, years, storages, cnt)[0])
    return np.concatenate(recs), W.reshape(-1)


def literal_variable_chain(seed: int, chain: int, cap, mttf, mttr, load, years: int, start: int, weather_out, weather_load=None,
                           resource_scale=None, pick: int = PICK_RANDOM, storages=(), scale: float = 1.0, shift: float = 0.0):
    """The contract of relmc_hl1_var_seq (include/relmc.h) as one plain loop, in Python floats: years and hours outside; units, then
    resources, then storages inside; no groups, lanes, bits or skipped steps.  The unit states are hl1_seq_model.literal_chain's hour
    loop (`ttf -= 1; while ttf <= 0: toggle, ttf += duration`); only the draws (SEQ.chronology's U) are shared with variable_model, and
    the weather year is weather_year's, one call per year.  -> (rec[years, 6], weather[years])."""
    out = np.asarray(weather_out, dtype=np.float64)
    nw, nres, H = out.shape
    K = len(cap)
    _, _, U = SEQ.chronology(seed, [chain], mttf, mttr, start, years * H)
    u, lnU = U[0].tolist(), np.log(U[0]).tolist()
    mttf, mttr, cap, load = ([float(x) for x in v] for v in (mttf, mttr, cap, load))
    out = out.tolist()
    wl = None if weather_load is None else np.asarray(weather_load, dtype=np.float64).tolist()
    rs = [1.0] * nres if resource_scale is None else [float(v) for v in resource_scale]
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
    rec = np.zeros((years, 6))
    weather = np.zeros(years, dtype=np.int64)
    was_loss = False
    for y in range(years):
        w = weather_year(seed, chain, y, years, nw, pick)
        weather[y] = w
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
            for r in range(nres):
                product = rs[r] * out[w][r][h]
                cap_avail = cap_avail + product
            base = wl[w][h] if wl is not None else load[h]
            product = scale * base
            L = product + shift
            loss = False
            if cap_avail < L:
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
                discharged += delivered
                if need > 0.0:
                    loss = True
                    lole += 1.0
                    eue += need
                    if not was_loss:
                        lolf += 1.0
                else:
                    served += 1.0
            elif cap_avail > L:
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
                charged += taken
            was_loss = loss
        rec[y] = (lole, eue, lolf, served, discharged, charged)
    return rec, weather
