"""Host model of the HL1 planning Monte Carlo (relmc_hl1_plan, include/relmc.h; generating_adequancy_comparative.jl:15-120,
tail_risk.jl:12-91).

  words / lfu_normal: the contract's draws.  Block b of hour h of year y = philox(ctr = (y_lo, y_hi, 0x20000000 | h, b), key = seed);
      z = sqrt(-2 ln U1) * cos(2 pi U2) from words 0 and 1; unit k is down iff word 2 + k < thr_k.
  model: vectorised over years.  The thermal capacity of every (year, hour) is an ordered sum over units; only the ELU energies chain
      the hours, so the hour loop runs over the ELU slots alone.  Also reports the (year, hour) pairs whose decision margin is within
      `tol` MW of zero: there a transcendental ulp of the device's log / cos could flip a decision.
  literal_year: a transliteration of the reference's hour loop in plain Python floats, fed the same words and normals.

The draws come from oracle.pyoracle.philox4x32_10 (imported, not changed).
"""
from __future__ import annotations

import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle.pyoracle import philox4x32_10  # noqa: E402

TAG = 0x20000000


def thresholds(for_rate) -> np.ndarray:
    t = np.floor(np.asarray(for_rate, dtype=np.float64) * 4294967296.0)
    return np.clip(np.where(t > 0, t, 0.0), 0.0, 4294967295.0).astype(np.uint64)


def words(seed: int, years, nhours: int, ngen: int) -> np.ndarray:
    """w[y, h, j]: word j of hour h of year years[y] (j < 4 * nblk, nblk = (ngen + 5) // 4)."""
    ys = np.asarray(years, dtype=np.uint64)
    nblk = (ngen + 5) // 4
    ctr = np.zeros((ys.size, nhours, nblk, 4), dtype=np.uint32)
    ctr[..., 0] = (ys & np.uint64(0xFFFFFFFF)).astype(np.uint32)[:, None, None]
    ctr[..., 1] = (ys >> np.uint64(32)).astype(np.uint32)[:, None, None]
    ctr[..., 2] = (np.arange(nhours, dtype=np.uint32) | np.uint32(TAG))[None, :, None]
    ctr[..., 3] = np.arange(nblk, dtype=np.uint32)[None, None, :]
    key = np.zeros((ys.size, nhours, nblk, 2), dtype=np.uint32)
    key[..., 0] = np.uint32(seed & 0xFFFFFFFF)
    key[..., 1] = np.uint32(seed >> 32)
    return philox4x32_10(ctr, key).reshape(ys.size, nhours, nblk * 4)


def lfu_normal(w) -> np.ndarray:
    u1 = (w[..., 0].astype(np.float64) + 0.5) * 2.0 ** -32
    u2 = (w[..., 1].astype(np.float64) + 0.5) * 2.0 ** -32
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)


def maintenance_hours(start, weeks, nhours: int):
    """[lo, hi) hour window per unit (start week 1-based, 0 = none), clipped to the year."""
    lo = np.zeros(len(start), dtype=np.int64)
    hi = np.zeros(len(start), dtype=np.int64)
    for k, (s, m) in enumerate(zip(start, weeks)):
        if s >= 1 and m >= 1:
            lo[k] = min((s - 1) * 168, nhours)
            hi[k] = min((s - 1 + m) * 168, nhours)
    return lo, hi


def model(seed, years, cap, for_rate, start, weeks, limit, load, sigma, tol=1e-6, chunk=64):
    """Per-year (loss hours, EUE, loss events), hour loss counts [H], ELU energies [Y, n_elu] and the number of near-tie decisions."""
    cap = np.asarray(cap, dtype=np.float64)
    limit = np.asarray(limit, dtype=np.float64)
    load = np.asarray(load, dtype=np.float64)
    years = np.asarray(years, dtype=np.uint64)
    K, H = cap.size, load.size
    thr = thresholds(for_rate)
    lo, hi = maintenance_hours(start, weeks, H)
    elu = [k for k in range(K) if limit[k] != math.inf]
    out = [np.zeros(years.size) for _ in range(3)]
    counts = np.zeros(H, dtype=np.int64)
    energy = np.zeros((years.size, len(elu)))
    ties = 0
    hours = np.arange(H)
    for c0 in range(0, years.size, chunk):
        ys = years[c0:c0 + chunk]
        Y = ys.size
        w = words(seed, ys, H, K)
        z = lfu_normal(w)
        ld = load[None, :] + z * sigma                                   # product and sum each rounded
        up = {}
        cap_unl = np.zeros((Y, H))
        for k in range(K):
            a = (w[:, :, 2 + k].astype(np.uint64) >= thr[k]) & ~((hours >= lo[k]) & (hours < hi[k]))[None, :]
            if k in elu:
                up[k] = a
            else:
                cap_unl = cap_unl + np.where(a, cap[k], 0.0)               # ascending unit order
        x = ld - cap_unl
        uns = np.maximum(x, 0.0)
        if not elu:
            f = uns > 0.0
            d = np.where(f, uns, 0.0)
            ties += int(np.count_nonzero(np.abs(x) < tol))
        else:
            f = np.zeros((Y, H), dtype=bool)
            d = np.zeros((Y, H))
            en = np.zeros((Y, len(elu)))
            for h in range(H):
                cap_elu = np.zeros(Y)
                av = np.zeros((Y, len(elu)), dtype=bool)
                for s, k in enumerate(elu):
                    av[:, s] = up[k][:, h] & ~(en[:, s] >= limit[k])
                    ties += int(np.count_nonzero(up[k][:, h] & (np.abs(en[:, s] - limit[k]) < tol)))
                    cap_elu = cap_elu + np.where(av[:, s], cap[k], 0.0)
                u = uns[:, h]
                fh = u > cap_elu
                ties += int(np.count_nonzero(np.abs(x[:, h] - cap_elu) < tol) + np.count_nonzero(np.abs(x[:, h]) < tol))
                part = ~fh & (u > 0.0)
                for s, k in enumerate(elu):
                    full = fh & av[:, s]
                    share = part & av[:, s]
                    en[:, s] = np.where(full, en[:, s] + cap[k], en[:, s])
                    with np.errstate(divide="ignore", invalid="ignore"):
                        en[:, s] = np.where(share, en[:, s] + u * (cap[k] / cap_elu), en[:, s])
                f[:, h] = fh
                d[:, h] = np.where(fh, u - cap_elu, 0.0)
            energy[c0:c0 + Y] = en
        out[0][c0:c0 + Y] = f.sum(axis=1)
        eue = np.zeros(Y)
        for h in range(H):                                                # hour order, as the lane sums
            eue = eue + d[:, h]
        out[1][c0:c0 + Y] = eue
        out[2][c0:c0 + Y] = (f & ~np.concatenate([np.zeros((Y, 1), dtype=bool), f[:, :-1]], axis=1)).sum(axis=1)
        counts += f.sum(axis=0)
    return out[0], out[1], out[2], counts, energy, ties


def literal_year(seed, year, cap, for_rate, start, weeks, limit, load, sigma):
    """The reference's hour loop (comparative.jl:34-117) for one year, plain Python floats, the contract's draws."""
    H, K = len(load), len(cap)
    w = words(seed, [year], H, K)[0]
    z = lfu_normal(w)
    thr = thresholds(for_rate)
    energy = [0.0] * K
    lole = eue = events = 0.0
    prev = False
    loss_hours = []
    elu_e = []
    for h in range(H):
        week = h // 168 + 1
        cap_unl = cap_elu = 0.0
        avail = []
        for i in range(K):
            if start[i] >= 1 and start[i] <= week < start[i] + weeks[i]:
                continue
            if int(w[h, 2 + i]) < int(thr[i]):
                continue
            if limit[i] != math.inf:
                if energy[i] >= limit[i]:
                    continue
                cap_elu += float(cap[i])
                avail.append(i)
            else:
                cap_unl += float(cap[i])
        actual = float(load[h]) + float(z[h]) * sigma
        unserved = max(0.0, actual - cap_unl)
        deficit = 0.0
        if unserved > 0:
            if unserved > cap_elu:
                deficit = unserved - cap_elu
                for i in avail:
                    energy[i] += float(cap[i])
            else:
                for i in avail:
                    energy[i] += unserved * (float(cap[i]) / cap_elu)
        loss = deficit > 0
        if loss:
            lole += 1.0
            eue += deficit
            loss_hours.append(h)
            if not prev:
                events += 1.0
        prev = loss
    elu_e = [energy[i] for i in range(K) if limit[i] != math.inf]
    return lole, eue, events, loss_hours, elu_e


def elu3_fleet():
    """12 units with non-integer capacities, 3 of them energy-limited, 600 hours, maintenance windows."""
    rng = np.random.default_rng(17)
    cap = np.round(rng.uniform(20.0, 120.0, 12), 3) + 0.137
    forr = rng.uniform(0.02, 0.12, 12)
    start = np.array([1, 0, 2, 0, 0, 3, 0, 1, 0, 0, 2, 0], dtype=np.int32)
    weeks = np.array([1, 0, 1, 0, 0, 1, 0, 2, 0, 0, 1, 0], dtype=np.int32)
    limit = np.full(12, math.inf)
    limit[[2, 6, 9]] = [12000.0, 5000.5, 9200.25]
    load = 0.62 * cap.sum() + 0.1 * cap.sum() * np.sin(np.arange(600) / 600.0 * 6.0 * np.pi)
    return cap, forr, start, weeks, limit, load


def fleet100():
    """100 units with non-integer capacities (two per Philox word group boundary and past 64 units), 3 ELUs, a 1000-hour year whose
    weeks 2..6 carry maintenance."""
    rng = np.random.default_rng(23)
    cap = np.round(rng.uniform(15.0, 160.0, 100), 2) + 0.013
    forr = rng.uniform(0.01, 0.1, 100)
    start = np.zeros(100, dtype=np.int32)
    weeks = np.zeros(100, dtype=np.int32)
    start[::9] = rng.integers(2, 6, start[::9].size)
    weeks[::9] = rng.integers(1, 3, weeks[::9].size)
    limit = np.full(100, math.inf)
    limit[[5, 50, 97]] = [3300.0, 1550.0, 3600.0]
    load = 0.80 * cap.sum() + 0.06 * cap.sum() * np.sin(np.arange(1000) / 1000.0 * 4.0 * np.pi)
    return cap, forr, start, weeks, limit, load
