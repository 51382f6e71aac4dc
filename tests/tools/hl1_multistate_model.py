"""Host model of the HL1 sequential chronology with three-state units (relmc_hl1_ms_load / relmc_hl1_ms_seq, include/relmc.h).

A fleet is a list of units (capacity_mw, derated_mw, mean_h[3], first_p[3]): the library's form, states 0 UP, 1 DERATED, 2 DOWN.

  (a) interval_chain / interval_model: the contract's interval form in numpy.  The sojourn that starts at T_j covers the steps n with
      T_j <= n < T_j+1; durations -mean_h[state] * ln U from hl1_seq_model's draw stream, T as running sums (product and sum each
      rounded), destinations from the second stream (k | 0x50000000), the stationary start from the contract's thresholds.
  (b) literal_chain: a plain hour loop (`t -= 1; while t <= 0: jump`) driven by the same draws, to cross-check (a).
  (c) exact expectations of a small fleet: stationary LOLE, EUE and loss events per year by enumerating the joint states of two
      consecutive hours; a unit's one-hour transition matrix is the 3x3 matrix exponential (scaling and squaring).
  path_counts: which of the chronology's edge cases a fixture reaches (sojourns that cover no step, DERATED -> DOWN -> DERATED inside
      one 64-step group, sojourns across a group edge, a window edge and a year boundary).
"""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle.pyoracle import philox4x32_10  # noqa: E402

_spec = importlib.util.spec_from_file_location("hl1_seq_model", os.path.join(ROOT, "tests", "tools", "hl1_seq_model.py"))
SEQ = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(SEQ)

ALL_UP, STATIONARY = SEQ.ALL_UP, SEQ.STATIONARY
DURATION_TAG, BRANCH_TAG = 0x40000000, 0x50000000
WINDOW = 256                                                       # HL1_MS_WINDOW of the kernel
DEST = np.array([[2, 1], [0, 2], [0, 1]])                          # of each state: first-listed destination, the other


def draws(seed: int, chains, nunits: int, nevents: int, tag: int) -> np.ndarray:
    """U[c, k, e] of draw e of unit k in chain chains[c] of the stream `tag`: (philox(ctr=(c_lo, c_hi, k | tag, e >> 2), key=seed)[e & 3] + 0.5) / 2^32."""
    ch = np.asarray(chains, dtype=np.uint64)
    nb = (nevents + 3) // 4
    ctr = np.zeros((ch.size, nunits, nb, 4), dtype=np.uint32)
    ctr[..., 0] = (ch & np.uint64(0xFFFFFFFF)).astype(np.uint32)[:, None, None]
    ctr[..., 1] = (ch >> np.uint64(32)).astype(np.uint32)[:, None, None]
    ctr[..., 2] = (np.arange(nunits, dtype=np.uint32) | np.uint32(tag))[None, :, None]
    ctr[..., 3] = np.arange(nb, dtype=np.uint32)[None, None, :]
    key = np.zeros((ch.size, nunits, nb, 2), dtype=np.uint32)
    key[..., 0] = np.uint32(seed & 0xFFFFFFFF)
    key[..., 1] = np.uint32(seed >> 32)
    w = philox4x32_10(ctr, key).reshape(ch.size, nunits, nb * 4)[..., :nevents]
    return (w.astype(np.float64) + 0.5) * 2.0 ** -32


def thresholds(unit) -> tuple:
    """The contract's stationary law of one unit -> (pi_2, pi_2 + pi_1, pi_1), over the states that can be reached from UP."""
    _, _, m, f = unit
    reach, todo = {0}, [0]
    while todo:
        s = todo.pop()
        for d, on in ((DEST[s][0], f[s] > 0.0), (DEST[s][1], f[s] < 1.0)):
            if on and int(d) not in reach:
                reach.add(int(d)); todo.append(int(d))
    if reach == {0, 1, 2}:
        nu0, nu1, nu2 = f[2] + f[1] * (1.0 - f[2]), (1.0 - f[2]) + f[2] * (1.0 - f[0]), (1.0 - f[1]) + f[1] * f[0]
        w0, w1, w2 = nu0 * m[0], nu1 * m[1], nu2 * m[2]
        tot = (w0 + w1) + w2
        return w2 / tot, w2 / tot + w1 / tot, w1 / tot
    if 2 in reach:
        q = m[2] / (m[0] + m[2])                                   # hl1_units_fill's expression
        return q, q, 0.0
    q = m[1] / (m[0] + m[1])
    return 0.0, q, q


def _arrays(units):
    cap = np.array([u[0] for u in units], dtype=np.float64)
    der = np.array([u[1] for u in units], dtype=np.float64)
    mean = np.array([u[2] for u in units], dtype=np.float64)
    fp = np.array([u[3] for u in units], dtype=np.float64)
    return cap, der, mean, fp


def chronology(seed: int, chains, units, start: int, nsteps: int):
    """States St[c, k, j] of sojourn j (j = 0: the start state), transition times T[c, k, j] = the end of sojourn j (running sums in
    event order), and the draws U (durations) and B (branches).  Enough events that every unit's last T exceeds nsteps."""
    _, _, mean, fp = _arrays(units)
    K = len(units)
    thr = np.array([thresholds(u)[:2] for u in units])
    kk = np.arange(K)[None, :]
    nev = 32
    while True:
        U = draws(seed, chains, K, nev, DURATION_TAG)
        B = draws(seed, chains, K, nev, BRANCH_TAG)
        if start == STATIONARY:
            u0 = U[:, :, 0]
            st = np.where(u0 < thr[None, :, 0], 2, np.where(u0 < thr[None, :, 1], 1, 0))
            first = 1
        else:
            st = np.zeros(U.shape[:2], dtype=np.int64)
            first = 0
        lnU = np.log(U)
        states, T, t = [st], [], None
        for e in range(first, nev):
            dur = (-mean[kk, st]) * lnU[:, :, e]
            t = dur if t is None else t + dur                      # T_1 = 0 + duration exactly; then one rounded sum per event
            T.append(t)
            take_first = B[:, :, e] < fp[kk, st]                   # U lies in (0, 1): first_p 1 always takes the first, 0 never
            st = np.where(take_first, DEST[st, 0], DEST[st, 1])
            states.append(st)
        T = np.stack(T, axis=2)
        if np.all(T[:, :, -1] > nsteps + 2):
            return np.stack(states, axis=2), T, U, B
        nev *= 2


def step_states(St_k, T_k, nsteps: int) -> np.ndarray:
    """One unit's state at the steps 1 .. nsteps."""
    n = np.arange(1, nsteps + 1, dtype=np.float64)
    return St_k[np.searchsorted(T_k, n, side="right")]             # #{T_j <= n} = the sojourn the step lies in


def interval_chain(St, T, units, load, years: int):
    """(a) One chain: St[K, E + 1], T[K, E] -> per-year arrays (loss hours, EUE, loss events, derated unit-hours, down unit-hours)."""
    cap, der, _, _ = _arrays(units)
    load = np.asarray(load, dtype=np.float64)
    H = load.size
    S = years * H
    cav, nder, ndown = np.zeros(S), np.zeros(S), np.zeros(S)
    for k in range(len(units)):                                    # ascending unit order, + 0.0 for a DOWN unit (exact)
        s = step_states(St[k], T[k], S)
        cav = cav + np.where(s == 2, 0.0, np.where(s == 1, der[k], cap[k]))
        nder += s == 1
        ndown += s == 2
    ld = np.tile(load, years)
    loss = cav < ld
    deficit = np.where(loss, ld - cav, 0.0)
    rise = loss & ~np.concatenate([[False], loss[:-1]])
    yr = lambda x: x.reshape(years, H).sum(1).astype(np.float64)
    return yr(loss), deficit.reshape(years, H).sum(1), yr(rise), yr(nder), yr(ndown)


def interval_model(seed: int, chains, units, load, years: int, start: int) -> np.ndarray:
    """(a) for chains `chains`: rec[nchains * years, 5] = (loss hours, EUE, loss events, derated unit-hours, down unit-hours), chain-major."""
    chains = np.atleast_1d(np.asarray(chains, dtype=np.uint64))
    H = np.asarray(load).size
    rows = []
    for c0 in range(0, chains.size, 64):
        St, T, _, _ = chronology(seed, chains[c0:c0 + 64], units, start, years * H)
        for c in range(St.shape[0]):
            rows.append(np.stack(interval_chain(St[c], T[c], units, load, years), axis=1))
    return np.concatenate(rows)


def literal_chain(seed: int, chain: int, units, load, years: int, start: int) -> np.ndarray:
    """(b) The hour loop outside, the unit loop inside, one chain, the contract's draws -> rec[years, 5]."""
    K, H = len(units), len(load)
    _, _, U, B = chronology(seed, [chain], units, start, years * H)
    u, lnU, br = U[0].tolist(), np.log(U[0]).tolist(), B[0].tolist()
    cap = [float(x[0]) for x in units]; der = [float(x[1]) for x in units]
    mean = [[float(v) for v in x[2]] for x in units]; fp = [[float(v) for v in x[3]] for x in units]
    load = [float(x) for x in load]
    state, t, ev = [0] * K, [0.0] * K, [0] * K
    for i in range(K):
        if start == STATIONARY:
            p2, p12, _ = thresholds(units[i])
            state[i] = 2 if u[i][0] < p2 else 1 if u[i][0] < p12 else 0
            ev[i] = 1
        t[i] = -mean[i][state[i]] * lnU[i][ev[i]]
        ev[i] += 1
    out = []
    was_loss = False
    for _y in range(years):
        rec = [0.0] * 5
        for h in range(H):
            cap_avail = 0.0
            for i in range(K):
                t[i] -= 1.0
                while t[i] <= 0:                                   # the jump that ends the sojourn timed by duration draw ev - 1
                    s = state[i]
                    state[i] = int(DEST[s][0] if br[i][ev[i] - 1] < fp[i][s] else DEST[s][1])
                    t[i] += -mean[i][state[i]] * lnU[i][ev[i]]
                    ev[i] += 1
                if state[i] == 0:
                    cap_avail += cap[i]
                elif state[i] == 1:
                    cap_avail += der[i]; rec[3] += 1.0
                else:
                    rec[4] += 1.0
            if cap_avail < load[h]:
                rec[0] += 1.0
                rec[1] += load[h] - cap_avail
                if not was_loss:
                    rec[2] += 1.0
                was_loss = True
            else:
                was_loss = False
        out.append(rec)
    return np.array(out)


def path_counts(seed: int, chains, units, load, years: int, start: int) -> dict:
    """Which edge cases of the chronology the chains reach, counted over the DERATED and DOWN sojourns that begin at or before the last
    step (a sojourn covers the steps a .. b - 1, a = ceil of its start, b = ceil of its end):
      zero           it covers no step (both ends round up to the same step)
      der_down_der   DERATED -> DOWN -> DERATED, each covering a step, the last step of the first and the first step of the third in
                     one 64-step group
      group / window / year   it covers steps on both sides of a group edge, a window edge, a year boundary."""
    H = np.asarray(load).size
    S = years * H
    out = dict(zero=0, der_down_der=0, group=0, window=0, year=0)
    St, T, _, _ = chronology(seed, np.atleast_1d(np.asarray(chains, dtype=np.uint64)), units, start, S)
    for c in range(St.shape[0]):
        for k in range(len(units)):
            ends = np.ceil(T[c, k]).astype(np.int64)
            a = np.concatenate([[1], ends[:-1]]); b = ends                  # sojourn j covers a[j] .. b[j] - 1
            a = np.maximum(a, 1)
            s = St[c, k, :-1]
            live = (s != 0) & (a <= S)
            b2 = np.minimum(b, S + 1)
            out["zero"] += int((live & (b == a)).sum())
            cov = live & (b2 > a)
            first, last = a - 1, b2 - 2                                     # 0-based first and last covered step
            out["group"] += int((cov & (first // 64 != last // 64)).sum())
            out["window"] += int((cov & (first // WINDOW != last // WINDOW)).sum())
            out["year"] += int((cov & (first // H != last // H)).sum())
            tri = cov[:-2] & cov[1:-1] & cov[2:] & (s[:-2] == 1) & (s[1:-1] == 2) & (s[2:] == 1)
            out["der_down_der"] += int((tri & (last[:-2] // 64 == first[2:] // 64)).sum())
    return out


# ---- (c) exact expectations ------------------------------------------------------------------------------------------------------
def generator_matrix(unit) -> np.ndarray:
    """Q of one unit: rate i -> j = the destination's share / mean_h[i], the diagonal = minus the row's sum."""
    _, _, m, f = unit
    Q = np.zeros((3, 3))
    for i in range(3):
        Q[i, DEST[i][0]] += f[i] / m[i]
        Q[i, DEST[i][1]] += (1.0 - f[i]) / m[i]
        Q[i, i] = -(Q[i].sum())
    return Q


def expm(A: np.ndarray) -> np.ndarray:
    """exp(A) by scaling and squaring: A / 2^s with norm below 1/4, a Taylor series to 1e-18, then s squarings."""
    A = np.asarray(A, dtype=np.float64)
    s = max(0, int(np.ceil(np.log2(max(np.abs(A).sum(1).max(), 1e-300)))) + 2)
    X = A / 2.0 ** s
    E, term = np.eye(A.shape[0]), np.eye(A.shape[0])
    for n in range(1, 30):
        term = term @ X / n
        E = E + term
        if np.abs(term).max() < 1e-18:
            break
    for _ in range(s):
        E = E @ E
    return E


def small_fleet_stationary(units, load):
    """Exact stationary LOLE, EUE and loss events of a one-year chain of a small fleet (<= 5 units) by enumerating its 3^K joint states:
    E[events] = P(loss at step 1) + sum_n P(no loss at n - 1, loss at n), the one-hour transition matrix the Kronecker product of the
    units' exp(Q)."""
    cap, der, _, _ = _arrays(units)
    load = np.asarray(load, dtype=np.float64)
    K = len(units)
    idx = np.stack(np.meshgrid(*[np.arange(3)] * K, indexing="ij"), axis=-1).reshape(-1, K)      # unit 0 outermost
    avail = np.zeros(idx.shape[0])
    pi = np.ones(idx.shape[0])
    M = np.ones((1, 1))
    for k in range(K):
        avail = avail + np.where(idx[:, k] == 2, 0.0, np.where(idx[:, k] == 1, der[k], cap[k]))
        p2, _, p1 = thresholds(units[k])
        pi = pi * np.array([1.0 - p1 - p2, p1, p2])[idx[:, k]]
        M = np.kron(M, expm(generator_matrix(units[k])))
    loss = avail[None, :] < load[:, None]
    lole = float((pi[None, :] * loss).sum())
    eue = float((pi[None, :] * loss * (load[:, None] - avail[None, :])).sum())

    def rise(a, b):
        return float(((pi * (avail >= a)) @ M)[avail < b].sum())

    lolf = float(pi[avail < load[0]].sum()) + sum(rise(load[n - 1], load[n]) for n in range(1, load.size))
    return lole, eue, lolf


# ---- fleets of the tests ---------------------------------------------------------------------------------------------------------
def two_state(cap, mttf, mttr) -> tuple:
    return (float(cap), 0.0, (float(mttf), 1.0, float(mttr)), (1.0, 1.0, 1.0))


def three_state(cap, der, mttf, mttr, scale=(1.0, 1.0, 2.0, 0.2, 1.0, 0.25)) -> tuple:
    """A derated unit from a two-state one's mttf / mttr: rates UP -> DERATED, UP -> DOWN = scale[0, 1] / mttf, DERATED -> UP, DERATED ->
    DOWN, DOWN -> UP, DOWN -> DERATED = scale[2 .. 5] / mttr."""
    l, m = 1.0 / mttf, 1.0 / mttr
    r01, r02, r10, r12, r20, r21 = scale[0] * l, scale[1] * l, scale[2] * m, scale[3] * m, scale[4] * m, scale[5] * m
    return (float(cap), float(der), (1.0 / (r01 + r02), 1.0 / (r10 + r12), 1.0 / (r20 + r21)),
            (r02 / (r01 + r02), r10 / (r10 + r12), r20 / (r20 + r21)))


def six_unit_fleet():
    """hl1_seq_model.small_fleet with units 0, 3 and 5 given a derated state at a non-integer capacity; one week of hourly load."""
    cap, mttf, mttr, load = SEQ.small_fleet()
    der = {0: 33.5, 3: 17.25, 5: 6.125}
    return [three_state(cap[k], der[k], mttf[k], mttr[k]) if k in der else two_state(cap[k], mttf[k], mttr[k]) for k in range(6)], load


def edge_fleet(n: int, nhours: int):
    """n units with non-integer capacities; those at indices 31, 32, 63 and 64 (the mask-word edge and the slot edge) and every
    eleventh one are derated.  The load curve sits about one unit below the mean available capacity."""
    rng = np.random.default_rng(20261020 + n)
    cap = np.round(rng.uniform(5.0, 60.0, n), 3) + 0.125
    mttf = rng.uniform(200.0, 1500.0, n)
    mttr = rng.uniform(10.0, 120.0, n)
    units = []
    for k in range(n):
        if k in (31, 32, 63, 64) or k % 11 == 5:
            units.append(three_state(cap[k], np.round(0.55 * cap[k], 3), mttf[k], mttr[k]))
        else:
            units.append(two_state(cap[k], mttf[k], mttr[k]))
    avail = 0.0
    for u in units:
        p2, _, p1 = thresholds(u)
        avail += (1.0 - p1 - p2) * u[0] + p1 * u[1]
    h = np.arange(nhours)
    load = avail * (0.93 + 0.04 * np.sin(2 * np.pi * h / 24.0) + 0.02 * np.sin(2 * np.pi * h / 97.0))
    return units, load


def short_fleet():
    """Eight units whose means are a few hours (some below one hour): sojourns that cover no step, several transitions inside one 64-step
    group, and, over a 300-hour year, sojourns across group edges, the window edge and the year boundary."""
    units = [(30.0, 12.5, (6.0, 2.5, 3.0), (0.3, 0.4, 0.5)),
             (25.0, 10.25, (9.0, 1.5, 0.8), (0.5, 0.2, 0.3)),      # DERATED leaves for DOWN four times in five, DOWN for DERATED mostly
             (20.0, 7.75, (4.0, 0.6, 5.0), (0.6, 0.7, 0.8)),
             (40.0, 20.0, (30.0, 40.0, 50.0), (0.5, 0.5, 0.5)),    # long sojourns: they cross the edges
             (15.0, 0.0, (12.0, 1.0, 2.0), (1.0, 1.0, 1.0)),       # two-state
             (10.0, 10.0, (5.0, 7.0, 1.0), (0.0, 1.0, 1.0)),       # UP <-> DERATED only, derated at full capacity
             (35.0, 17.5, (20.0, 3.0, 6.0), (0.4, 0.3, 0.0)),      # DOWN always leaves for DERATED; UP is regained from DERATED only
             (22.0, 11.0, (8.0, 2.0, 2.0), (1.0, 0.5, 0.0))]       # DERATED is reached through DOWN only
    h = np.arange(300)
    load = 120.0 + 25.0 * np.sin(2 * np.pi * h / 24.0)
    return units, load


def lolf_fleet():
    """Four three-state units (81 joint states) against hl1_seq_model.small_fleet's week: losses every few days."""
    _, _, _, load = SEQ.small_fleet()
    units = [three_state(70.0, 35.0, 400.0, 40.0), three_state(60.0, 30.0, 300.0, 30.0), three_state(55.0, 20.0, 350.0, 50.0),
             three_state(45.0, 22.5, 250.0, 20.0, scale=(2.0, 1.0, 1.0, 0.5, 1.0, 0.0))]
    return units, load
