"""Host model of weather-dependent forced outage rates on the HL1 sequential chronology (relmc_hl1_stress_seq, contract in include/relmc.h).

A UP unit of outage class c fails with the hazard fail_mult[w(y)][c][h] / mttf in hour h of chain year y.  The draws are the sequential
model's (hl1_seq_model.draws), the weather years, the capacity and load curves and the step loop over the storages are
hl1_variable_model's (weather_years, step_curves, variable_chain), cap_avail is hl1_storage_model's.  What is this model's own:

  cumulative         G[0] = 0, G[j + 1] = G[j] + fail_mult[j], one rounded addition per hour
  failure_time       the contract's "Failure time", operation for operation, in Python floats (each operation rounded once)
  stress_chronology  the start states and transition times of every unit: T + E for a repair and for a unit of class -1, failure_time
                     for a unit of a class that has just become UP
  stress_model       the records of chains, as hl1_variable_model.variable_model gives them

literal_stress_chain restates the model as one plain hour loop on the multipliers themselves (no cumulative table, no search, no walk
over the years): in every hour a UP unit of a class spends fail_mult[w][c][h] * (the part of the hour it is UP) of its draw, and fails
where the draw runs out.  It rounds differently, so tests/test_hl1_stress_host.py compares the per-year integers of small cases.

hourly_down_probability is the exact recursion for one unit started UP: within an hour the rates are constant.
"""
import importlib.util
import math
import os

import numpy as np

_spec = importlib.util.spec_from_file_location("hl1_variable_model", os.path.join(os.path.dirname(os.path.abspath(__file__)), "hl1_variable_model.py"))
VM = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(VM)
SM, SEQ = VM.SM, VM.SEQ

PICK_RANDOM, PICK_CYCLE = VM.PICK_RANDOM, VM.PICK_CYCLE


def cumulative(mult_row) -> np.ndarray:
    """G[0 .. H] of one row of multipliers."""
    g = [0.0]
    for m in np.asarray(mult_row, dtype=np.float64).tolist():
        g.append(g[-1] + m)
    return np.array(g)


def cumulative_tables(fail_mult) -> np.ndarray:
    """G[n_weather, n_classes, H + 1] of fail_mult[n_weather, n_classes, H]."""
    m = np.asarray(fail_mult, dtype=np.float64)
    return np.array([[cumulative(m[w, c]) for c in range(m.shape[1])] for w in range(m.shape[0])]).reshape(m.shape[0], m.shape[1], m.shape[2] + 1)


def failure_time(T: float, E: float, H: int, years: int, weather, G, cnt=None) -> float:
    """The chain time at which a unit that became UP at T fails, given the draw E; years * H + 1 if not within the chain.  weather[years]:
    the weather year of every chain year; G[w]: the cumulative table (a list of H + 1 Python floats) of the unit's class in weather year w.
    cnt: an optional dict that counts the paths taken: `carried` (the draw outlasts a year and goes on in the next one), `flat` (the
    search lands on an hour without slope, d == 0: the unit fails at that hour's end) and `immediate` (the unit fails within the hour in
    which it became UP)."""
    T, E = float(T), float(E)
    never = float(years * H + 1)
    if not T < float(years * H):
        return T if T > never else never
    n0 = int(T)                                                    # floor: T >= 0
    y, j = divmod(n0, H)
    g = G[weather[y]]
    frac = T - float(n0)
    slope = g[j + 1] - g[j]
    part = slope * frac
    a = g[j] + part
    rem = g[H] - a
    while E > rem:
        E = E - rem
        y += 1
        if y == years:
            return never
        if cnt is not None:
            cnt["carried"] += 1
        g = G[weather[y]]
        j, a, rem = 0, 0.0, g[H]
    t = a + E
    lo, hi = j, H - 1
    while lo < hi:
        mid = (lo + hi) >> 1
        if g[mid + 1] >= t:
            hi = mid
        else:
            lo = mid + 1
    g0 = g[lo]
    d = g[lo + 1] - g0
    f = 1.0
    if d > 0.0:
        num = t - g0
        f = num / d
        f = 0.0 if f < 0.0 else 1.0 if f > 1.0 else f
    if cnt is not None:
        cnt["flat"] += not d > 0.0
        cnt["immediate"] += y * H + lo == n0
    r = float(y * H + lo) + f
    return r if r > T else T


def stress_chronology(seed: int, chains, mttf, mttr, start: int, H: int, years: int, W, G, unit_class, counters=None):
    """Start states down0[c, k] and transition times T[c, k, :] (padded with inf behind the first time beyond the chain) of the chains
    `chains`, whose weather years are W[c, :].  G[n_weather, n_classes, H + 1].  counters: an optional dict that counts the transitions
    (`failures` through failure_time, `never` of them beyond the chain, `plain` the others, `plain_failures` those of the others that
    are failures of a unit of class -1; `carried`, `flat` and `immediate` as failure_time counts them)."""
    mttf, mttr = [float(v) for v in mttf], [float(v) for v in mttr]
    K, nsteps = len(mttf), years * H
    chains = np.atleast_1d(np.asarray(chains, dtype=np.uint64))
    Gl = [[row.tolist() for row in Gw] for Gw in np.asarray(G, dtype=np.float64).transpose(1, 0, 2)]       # [class][weather][H + 1]
    cls = [int(c) for c in unit_class]
    nev = int(2.5 * nsteps / min(f + r for f, r in zip(mttf, mttr)) * 2) + 16
    while True:
        U = SEQ.draws(seed, chains, K, nev)
        lnU = np.log(U)
        down0 = np.zeros((chains.size, K), dtype=bool)
        times, short = [], False
        cnt = dict(failures=0, never=0, plain=0, plain_failures=0, carried=0, flat=0, immediate=0)
        for c in range(chains.size):
            wy = [int(v) for v in W[c]]
            row = []
            for k in range(K):
                u, l = U[c, k].tolist(), lnU[c, k].tolist()
                down, ev = False, 0
                if start == SEQ.STATIONARY:
                    down, ev = u[0] < mttr[k] / (mttf[k] + mttr[k]), 1
                down0[c, k] = down
                T, ts = 0.0, []
                while True:
                    if ev >= nev:
                        short = True
                        break
                    e = -(mttr[k] if down else mttf[k]) * l[ev]
                    if not down and cls[k] >= 0:
                        T = failure_time(T, e, H, years, wy, Gl[cls[k]], cnt)
                        cnt["failures"] += 1
                        cnt["never"] += T == float(nsteps + 1)
                    else:
                        T = T + e
                        cnt["plain"] += 1
                        cnt["plain_failures"] += not down
                    ts.append(T)
                    down, ev = not down, ev + 1
                    if T > nsteps:
                        break
                row.append(ts)
            times.append(row)
        if not short:
            break
        nev *= 2
    if counters is not None:
        for key, v in cnt.items():
            counters[key] = counters.get(key, 0) + int(v)
    E = max(len(ts) for row in times for ts in row)
    T = np.full((chains.size, K, E), np.inf)
    for c, row in enumerate(times):
        for k, ts in enumerate(row):
            T[c, k, :len(ts)] = ts
    return down0, T


def stress_model(seed: int, chains, cap, mttf, mttr, load, years: int, start: int, weather_out, fail_mult, unit_class, weather_load=None,
                 resource_scale=None, pick: int = PICK_RANDOM, storages=(), scale: float = 1.0, shift: float = 0.0, counters=None,
                 step_counters=None, weather=None):
    """Chains `chains` -> (rec[nchains * years, 6], weather[nchains * years]), as hl1_variable_model.variable_model.
    fail_mult[n_weather, n_classes, H]; unit_class[K] in -1 .. n_classes - 1.  counters: stress_chronology's; step_counters:
    hl1_storage_model's, of the step loop; weather: as hl1_variable_model.variable_model's."""
    chains = np.atleast_1d(np.asarray(chains, dtype=np.uint64))
    out = np.asarray(weather_out, dtype=np.float64)
    nw, nres, H = out.shape
    rs = [1.0] * nres if resource_scale is None else [float(v) for v in resource_scale][:nres]
    W = VM.weather_years(seed, chains, years, nw, pick) if weather is None else np.asarray(weather, dtype=np.int64).reshape(chains.size, years)
    G = cumulative_tables(fail_mult)
    recs = []
    for c0 in range(0, chains.size, 256):
        down0, T = stress_chronology(seed, chains[c0:c0 + 256], mttf, mttr, start, H, years, W[c0:c0 + 256], G, unit_class, counters)
        for c in range(down0.shape[0]):
            cav = SM.cap_avail(down0[c], T[c], cap, years * H)
            cs, Ls = VM.step_curves(cav, W[c0 + c], load, out, weather_load, rs, scale, shift)
            recs.append(VM.variable_chain(cs, Ls, H, years, storages, step_counters)[0])
    return np.concatenate(recs), W.reshape(-1)


def literal_stress_chain(seed: int, chain: int, cap, mttf, mttr, load, years: int, start: int, weather_out, fail_mult, unit_class,
                         weather_load=None, resource_scale=None, pick: int = PICK_RANDOM, scale: float = 1.0, shift: float = 0.0):
    """The model as one plain hour loop without storages, on the multipliers themselves: years and hours outside, units inside.  A unit
    that is DOWN, or of class -1, keeps the time of its next transition (T + duration).  A UP unit of a class keeps what is left of its
    draw (`hz`) and the part of the current hour that had passed when it became UP (`pos`): in hour h it spends
    fail_mult[w][c][h] * (1 - pos); if the draw runs out inside the hour, it fails at that point of the hour.  Only the draws are shared
    with stress_model.  -> (rec[years, 3] = lole, eue, lolf per year, weather[years])."""
    out = np.asarray(weather_out, dtype=np.float64)
    nw, nres, H = out.shape
    K = len(cap)
    nev = int(2.5 * years * H / float(np.min(np.asarray(mttf) + np.asarray(mttr))) * 2) * 4 + 64
    U = SEQ.draws(seed, [chain], K, nev)
    u, lnU = U[0].tolist(), np.log(U[0]).tolist()
    mttf, mttr, cap, load = ([float(x) for x in v] for v in (mttf, mttr, cap, load))
    mult = np.asarray(fail_mult, dtype=np.float64).tolist()
    cls = [int(c) for c in unit_class]
    out = out.tolist()
    wl = None if weather_load is None else np.asarray(weather_load, dtype=np.float64).tolist()
    rs = [1.0] * nres if resource_scale is None else [float(v) for v in resource_scale]
    up, tn, hz, pos, ev = [True] * K, [0.0] * K, [0.0] * K, [0.0] * K, [0] * K
    for i in range(K):
        if start == SEQ.STATIONARY:
            up[i] = not (u[i][0] < mttr[i] / (mttf[i] + mttr[i]))
            ev[i] = 1
        d = -(mttf[i] if up[i] else mttr[i]) * lnU[i][ev[i]]
        ev[i] += 1
        if up[i] and cls[i] >= 0:
            hz[i], pos[i] = d, 0.0
        else:
            tn[i] = d
    rec = np.zeros((years, 3))
    weather = np.zeros(years, dtype=np.int64)
    was_loss = False
    for y in range(years):
        w = VM.weather_year(seed, chain, y, years, nw, pick)
        weather[y] = w
        for h in range(H):
            n = y * H + h + 1                                      # the step: the hour (n - 1, n]
            cap_avail = 0.0
            for i in range(K):
                while True:
                    if up[i] and cls[i] >= 0:
                        m = mult[w][cls[i]][h]
                        avail = m * (1.0 - pos[i])
                        if m > 0.0 and hz[i] <= avail:             # the draw runs out inside this hour
                            t_fail = (n - 1) + (pos[i] + hz[i] / m)
                            up[i] = False
                            tn[i] = t_fail + -mttr[i] * lnU[i][ev[i]]
                            ev[i] += 1
                            continue
                        hz[i] -= avail
                        pos[i] = 0.0
                        break
                    if tn[i] <= n:
                        up[i] = not up[i]
                        d = -(mttf[i] if up[i] else mttr[i]) * lnU[i][ev[i]]
                        ev[i] += 1
                        if up[i] and cls[i] >= 0:
                            hz[i], pos[i] = d, tn[i] - (n - 1)
                        else:
                            tn[i] += d
                        continue
                    break
                if up[i]:
                    cap_avail += cap[i]
            for r in range(nres):
                product = rs[r] * out[w][r][h]
                cap_avail = cap_avail + product
            base = wl[w][h] if wl is not None else load[h]
            product = scale * base
            L = product + shift
            loss = cap_avail < L
            if loss:
                rec[y, 0] += 1.0
                rec[y, 1] += L - cap_avail
                if not was_loss:
                    rec[y, 2] += 1.0
            was_loss = loss
    return rec, weather


def hourly_down_probability(mult_row, mttf: float, mttr: float) -> np.ndarray:
    """P(DOWN at step n), n = 1 .. H, of one unit started UP whose hazard in hour n - 1 is mult_row[n - 1] / mttf: within an hour the rates
    are constant, so p_n = p_inf + (p_(n-1) - p_inf) * exp(-(lam + mu)) with lam = mult / mttf, mu = 1 / mttr, p_inf = lam / (lam + mu)."""
    p, res = 0.0, []
    for m in np.asarray(mult_row, dtype=np.float64).tolist():
        lam, mu = m / mttf, 1.0 / mttr
        pinf = lam / (lam + mu)
        p = pinf + (p - pinf) * math.exp(-(lam + mu))
        res.append(p)
    return np.array(res)


# ---- libraries of the tests ------------------------------------------------------------------------------------------------------
def edge_multipliers(H: int = 200) -> np.ndarray:
    """fail_mult[3, 2, H] for small_fleet: class 0 varies between 0.25 and 3 in steps of 1/8, with zero stretches at the start, in the
    middle and at the end of weather year 0, weather year 1 all zero, and in weather year 2 one hour at 50 (several sojourns of a
    unit with a short repair end inside it); class 1 is 2^-24 in every hour, so small that no unit of it fails before a chain ends."""
    rng = np.random.default_rng(20261020)
    m = np.zeros((3, 2, H))
    m[:, 0, :] = rng.integers(2, 25, (3, H)) / 8.0
    m[0, 0, :17] = 0.0
    m[0, 0, H // 2 - 9:H // 2 + 12] = 0.0
    m[0, 0, H - 23:] = 0.0
    m[1, 0, :] = 0.0
    m[2, 0, H // 3] = 50.0
    m[:, 1, :] = 2.0 ** -24
    return m


def varying_multipliers(n_weather: int, n_classes: int, H: int, seed: int) -> np.ndarray:
    """fail_mult[n_weather, n_classes, H]: a daily wave times a slow random level, 0.2 .. 4, not rounded (every addition of G rounds)."""
    rng = np.random.default_rng(seed)
    h = np.arange(H)
    level = np.exp(rng.normal(0.0, 0.5, (n_weather, n_classes, (H + 47) // 48)))
    wave = 1.0 + 0.6 * np.sin(2.0 * np.pi * (h[None, None, :] / 24.0 + rng.uniform(0.0, 1.0, (n_weather, n_classes, 1))))
    return np.clip(np.repeat(level, 48, axis=2)[:, :, :H] * wave, 0.2, 4.0)
