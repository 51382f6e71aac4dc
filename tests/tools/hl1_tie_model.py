"""Host model of the HL1 multi-area chronology with tie outages (relmc_hl1_area_tie_outages, include/relmc.h).

  (a) interval_model: hl1_area_model.interval_model with a chronology per tie.  Tie t is component 128 + t of hl1_seq_model's draws; its
      start state and transition times come from hl1_seq_model.chronology itself (one chronology, not two).  Per step T is summed from
      0.0 over the UP ties in ascending tie order; the steps in deficit go through hl1_area_model.solve_batch with their own T.
  (b) literal_chain: the reference's hour loop (`ttf -= 1; while ttf <= 0: toggle`) for units and ties alike, driven by the same draws.
  (c) joint_stationary_ties: exact stationary LOLE / EUE per row as the sum over the 2^n_ties tie states of P(state) x
      hl1_area_model.joint_stationary(..., T(state), ...).  Exact because tie states are independent of the fleets and LOLE / EUE are
      sums of per-hour expectations; it says nothing about LOLF.
A tie with mttf = inf never fails and takes no draws.
"""
from __future__ import annotations

import importlib.util
import itertools
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
_spec = importlib.util.spec_from_file_location("hl1_area_model", os.path.join(ROOT, "tests", "tools", "hl1_area_model.py"))
AM = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(AM)
SEQ = AM.SEQ

ALL_UP, STATIONARY = AM.ALL_UP, AM.STATIONARY
ISOLATED, INTERCONNECTED = AM.ISOLATED, AM.INTERCONNECTED
REFERENCE, MAX_FLOW = AM.REFERENCE, AM.MAX_FLOW
DRAW_BASE = 128                       # RELMC_HL1_TIE_DRAW_BASE
_IDLE = (1e30, 1.0)                   # (mttf, mttr) of the component indices below 128 + t that the helper walks but nobody reads


def topology_up(n, ties, up):
    """T of a step: from 0.0, the capacities of the 0-based ties (from, to, capacity) with up[t], in ascending tie order."""
    return AM.topology(n, [tie for tie, u in zip(ties, up) if u])


def tie_chronology(seed, chains, tie_mttf, tie_mttr, start, nsteps):
    """hl1_seq_model.chronology for the ties as components 128 + t: (down0[c, t], T[c, t, :], U[c, t, :]).  A tie with mttf = inf is UP
    for ever: down0 False, every T = inf."""
    tie_mttf, tie_mttr = np.asarray(tie_mttf, dtype=np.float64), np.asarray(tie_mttr, dtype=np.float64)
    fails = np.isfinite(tie_mttf)
    mf = np.concatenate([np.full(DRAW_BASE, _IDLE[0]), np.where(fails, tie_mttf, _IDLE[0])])
    mr = np.concatenate([np.full(DRAW_BASE, _IDLE[1]), np.where(fails, tie_mttr, _IDLE[1])])
    down0, T, U = SEQ.chronology(seed, chains, mf, mr, start, nsteps)
    down0, T, U = down0[:, DRAW_BASE:].copy(), T[:, DRAW_BASE:].copy(), U[:, DRAW_BASE:]
    down0[:, ~fails] = False
    T[:, ~fails] = np.inf
    return down0, T, U


def tie_down(seed, chains, tie_mttf, tie_mttr, start, nsteps):
    """down[c, t, step - 1]: tie t DOWN at step 1 .. nsteps (start state toggled once per T_j <= step)."""
    down0, T, _ = tie_chronology(seed, chains, tie_mttf, tie_mttr, start, nsteps)
    steps = np.arange(1, nsteps + 1, dtype=np.float64)
    out = np.zeros(down0.shape + (nsteps,), dtype=bool)
    for c in range(down0.shape[0]):
        for t in range(down0.shape[1]):
            out[c, t] = down0[c, t] ^ (np.searchsorted(T[c, t], steps, side="right") & 1).astype(bool)
    return out


def unit_down(seed, chains, mttf, mttr, start, nsteps):
    """down[c, k, step - 1] of the units (hl1_seq_model.chronology with the global unit index)."""
    down0, T, _ = SEQ.chronology(seed, chains, mttf, mttr, start, nsteps)
    steps = np.arange(1, nsteps + 1, dtype=np.float64)
    out = np.zeros(down0.shape + (nsteps,), dtype=bool)
    for c in range(down0.shape[0]):
        for k in range(down0.shape[1]):
            out[c, k] = down0[c, k] ^ (np.searchsorted(T[c, k], steps, side="right") & 1).astype(bool)
    return out


def solve_steps(m, n, ties, tdown, policy, flow):
    """Curtailments c[S, n] of the margins m[S, n] with tdown[t, S] the ties' DOWN flags: the per-step rule of include/relmc.h.  Steps
    with every m_i >= 0 curtail nothing whatever the ties' states; the others go through one solve_batch call with a T per step."""
    if policy != INTERCONNECTED or len(ties) == 0:
        return AM.solve_batch(m, AM.topology(n, ties), policy, flow)
    c = np.zeros_like(m)
    idx = np.nonzero((m < 0).any(1))[0]
    T = np.zeros((idx.size, n, n))
    for t, (i, j, cap) in enumerate(ties):                         # from 0.0 in ascending tie order; + 0.0 for a DOWN tie is exact
        up = np.where(tdown[t][idx], 0.0, float(cap))
        T[:, i, j] += up
        T[:, j, i] += up
    c[idx] = AM.solve_batch(m[idx], T, policy, flow)
    return c


def interval_model(seed, chains, units_per_area, cap, mttf, mttr, loads, ties, tie_mttf, tie_mttr, years, start, policy, flow=REFERENCE):
    """(a): [len(chains) * years, n + 1, 3] in chain-major order.  ties: 0-based (from, to, capacity); tie_mttf / tie_mttr per tie."""
    chains = np.atleast_1d(np.asarray(chains, dtype=np.uint64))
    loads = np.atleast_2d(np.asarray(loads, dtype=np.float64))
    n, H = loads.shape
    S = years * H
    lo = np.concatenate([[0], np.cumsum(units_per_area)])
    hour = np.arange(S) % H
    out = []
    for c0 in range(0, chains.size, 32):
        ch = chains[c0:c0 + 32]
        ud = unit_down(seed, ch, mttf, mttr, start, S)
        td = tie_down(seed, ch, tie_mttf, tie_mttr, start, S) if len(ties) else np.zeros((ch.size, 0, S), dtype=bool)
        for c in range(ch.size):
            m = np.zeros((S, n))
            for a in range(n):
                cav = np.zeros(S)
                for k in range(lo[a], lo[a + 1]):                  # ascending units, + 0.0 for a DOWN unit (exact)
                    cav = cav + np.where(ud[c, k], 0.0, float(cap[k]))
                m[:, a] = cav - loads[a][hour]
            out.append(AM._rows(solve_steps(m, n, ties, td[c], policy, flow), years, H))
    return np.concatenate(out)


def literal_chain(seed, chain, units_per_area, cap, mttf, mttr, loads, ties, tie_mttf, tie_mttr, years, start, policy, flow=REFERENCE):
    """(b) one chain: the hour loop with `ttf -= 1` for every unit and every failing tie -> [years, n + 1, 3]."""
    loads = [[float(x) for x in row] for row in np.atleast_2d(loads)]
    n, H = len(loads), len(loads[0])
    K, nt = len(cap), len(ties)
    S = years * H
    _, _, Uu = SEQ.chronology(seed, [chain], mttf, mttr, start, S)
    Ut = tie_chronology(seed, [chain], tie_mttf, tie_mttr, start, S)[2] if nt else np.zeros((1, 0, 1))
    # components: units, then the failing ties; each with its own (mttf, mttr) and draws
    fails = [t for t in range(nt) if np.isfinite(tie_mttf[t])]
    cf = [float(x) for x in mttf] + [float(tie_mttf[t]) for t in fails]
    cr = [float(x) for x in mttr] + [float(tie_mttr[t]) for t in fails]
    u = Uu[0].tolist() + [Ut[0, t].tolist() for t in fails]
    lnU = np.log(Uu[0]).tolist() + [np.log(Ut[0, t]).tolist() for t in fails]
    cap = [float(x) for x in cap]
    lo = [0] + list(np.cumsum(units_per_area))
    N = K + len(fails)
    status, ttf, ev = [True] * N, [0.0] * N, [0] * N
    for i in range(N):
        if start == STATIONARY:
            status[i] = not (u[i][0] < cr[i] / (cf[i] + cr[i]))
            ev[i] = 1
        ttf[i] = -(cf[i] if status[i] else cr[i]) * lnU[i][ev[i]]
        ev[i] += 1

    def step(i):
        ttf[i] -= 1.0
        while ttf[i] <= 0:
            status[i] = not status[i]
            ttf[i] += -(cf[i] if status[i] else cr[i]) * lnU[i][ev[i]]
            ev[i] += 1
        return status[i]

    out = np.zeros((years, n + 1, 3))
    was = [False] * (n + 1)
    for y in range(years):
        for h in range(H):
            margins = [0.0] * (n + 1)
            for a in range(n):
                area_cap = 0.0
                for g in range(lo[a], lo[a + 1]):
                    if step(g):
                        area_cap += cap[g]
                margins[a + 1] = area_cap - loads[a][h]
            up = [True] * nt
            for j, t in enumerate(fails):
                up[t] = step(K + j)
            if all(x >= 0 for x in margins[1:]):
                curt = [0.0] * n
            elif policy == ISOLATED or flow == REFERENCE:
                T = topology_up(n, ties, up)
                topo = [[0.0] * (n + 1)] + [[0.0] + [float(x) for x in row] for row in T]
                curt = AM._solve_literal(topo, margins, policy)[1:]
            else:
                curt = AM.solve_batch(np.array([margins[1:]]), topology_up(n, ties, up), policy, flow)[0].tolist()
            ds = 0.0
            for a in range(n):
                ds += curt[a]
            flags = [c > 0 for c in curt]
            flags.append(any(flags))
            vals = curt + [ds]
            for r in range(n + 1):
                if flags[r]:
                    out[y, r, 0] += 1.0
                    out[y, r, 1] += vals[r]
                    if not was[r]:
                        out[y, r, 2] += 1.0
                was[r] = flags[r]
    return out


def joint_stationary_ties(units_per_area, cap_int, mttf, mttr, loads, ties, tie_mttf, tie_mttr, policy, flow=REFERENCE):
    """(c): exact stationary annual (LOLE, EUE) per row [n + 1, 2]: sum over the tie states of P(state) x joint_stationary(T(state))."""
    n = np.atleast_2d(np.asarray(loads)).shape[0]
    tie_mttf, tie_mttr = np.asarray(tie_mttf, dtype=np.float64), np.asarray(tie_mttr, dtype=np.float64)
    fails = [t for t in range(len(ties)) if np.isfinite(tie_mttf[t])]
    out = np.zeros((n + 1, 2))
    for state in itertools.product((True, False), repeat=len(fails)):          # True: UP
        up, p = [True] * len(ties), 1.0
        for t, s in zip(fails, state):
            q = tie_mttr[t] / (tie_mttf[t] + tie_mttr[t])
            up[t] = s
            p *= (1.0 - q) if s else q
        out += p * AM.joint_stationary(units_per_area, cap_int, mttf, mttr, loads, topology_up(n, ties, up), policy, flow)
    return out
