"""Plain reference of the unique-state database's sums (nsqMain.m:282-301, 348-349, 366-376 over database rows) and generators of the rows the
device kernels are tested on.  TEST TOOL: numpy + Python integers, nothing taken from the library.

  accumulate(rows)              the accumulators of a row set: integers exact, fp64 sums correct to far below one ulp of their magnitude sum
  unique_stable(states)         distinct rows of a sampled state matrix in order of first appearance, with multiplicities (unique(..., 'stable'))
  synthetic_rows(case, R, seed) R rows with pairwise distinct masks whose contents sit on every comparison and bit edge of the reduction kernel

Rows are dicts of arrays: states[R, ncomp] (0/1), count[R], dns[R], nodal[R, nb], status[R] (0..3), iters[R], relaxed[R] (bit 0: island rule
relaxed, bit 1: certified by the pre-screen).
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

EDGE_BITS = (0, 31, 32, 63, 64)          # + ncomp - 1: first / last bit of the 32-bit mask words and of the 64-bit sort chunks
FRACTION_ROWS = 4096                     # up to here the fp64 sums are rational arithmetic; above, compensated long-double sums
DNS_CLASSES = ("large", "threshold", "above_threshold", "below_threshold", "negative", "zero")


def _exact_sum(w, x):
    """sum_r w[r] * x[r] for integer weights w (< 2^53) and doubles x, as the double nearest to the exact value (or within 2^-63 relative to
    sum |w x| of it): Fractions for small sets; otherwise every product in 64-bit-mantissa long double (a 41-bit count times a 53-bit double
    needs 94 bits: one rounding of 2^-64 relative), split into two doubles, and math.fsum -- which is exact -- over all the halves."""
    w = np.asarray(w); x = np.asarray(x, dtype=np.float64)
    if w.size == 0:
        return 0.0
    if w.size <= FRACTION_ROWS or np.finfo(np.longdouble).nmant < 63:
        return float(sum((Fraction(int(a)) * Fraction(float(b)) for a, b in zip(w.tolist(), x.tolist())), Fraction(0)))
    p = w.astype(np.longdouble) * x.astype(np.longdouble)
    hi = p.astype(np.float64)
    lo = (p - hi.astype(np.longdouble)).astype(np.float64)
    return math.fsum(np.concatenate([hi, lo]).tolist())


def _exact_sum_sq(w, x):
    """sum_r w[r] * x[r]^2, same accuracy class (two long-double roundings per term on the large sets)."""
    w = np.asarray(w); x = np.asarray(x, dtype=np.float64)
    if w.size == 0:
        return 0.0
    if w.size <= FRACTION_ROWS or np.finfo(np.longdouble).nmant < 63:
        return float(sum((Fraction(int(a)) * Fraction(float(b)) ** 2 for a, b in zip(w.tolist(), x.tolist())), Fraction(0)))
    xl = x.astype(np.longdouble)
    p = w.astype(np.longdouble) * xl * xl
    hi = p.astype(np.float64)
    lo = (p - hi.astype(np.longdouble)).astype(np.float64)
    return math.fsum(np.concatenate([hi, lo]).tolist())


def accumulate(rows, fail_threshold=1e-4):
    """The accumulators of include/relmc.h's relmc_acc from database rows.  Four different comparisons on dns, as the reference has them:
    `!= 0` for the moments, `> fail_threshold` for the failure count and the component counts (nsqMain.m:270), `> 0` for the nodal sums
    (mc_simulation.m:65), and the status / relaxed columns for the solver counters.  Also T1, T2, Tb: the sums of the magnitudes of the terms
    of sum_dns, sum_dns2, sum_nodal[b], which scale the rounding tolerance of an fp64 summation of the same terms."""
    st = np.asarray(rows["states"]); c = np.asarray(rows["count"], dtype=np.int64)
    d = np.asarray(rows["dns"], dtype=np.float64); nod = np.asarray(rows["nodal"], dtype=np.float64)
    R = c.size
    zeros = np.zeros(R, dtype=np.int64)
    status = np.asarray(rows.get("status", zeros)).astype(np.int64)
    iters = np.asarray(rows.get("iters", zeros)).astype(np.int64)
    relaxed = np.asarray(rows.get("relaxed", zeros)).astype(np.int64)
    assert R == 0 or int(c.max()) < 2 ** 53
    isum = lambda sel: sum(c[sel].tolist())                           # Python integers: no overflow, no rounding
    fail = d > fail_threshold
    out = dict(
        n=isum(slice(None)), n_fail=isum(fail), n_singular=isum(status == 3), n_nonconverged=isum((status == 1) | (status == 2)),
        n_infeasible=isum((relaxed & 1) != 0), n_screened=isum((relaxed & 2) != 0),
        sum_iters=sum(int(a) * int(b) for a, b in zip(c.tolist(), iters.tolist())))
    assert out["sum_iters"] < 2 ** 63
    cf, stf = c[fail], st[fail] != 0
    out["comp_fail"] = [int(cf[stf[:, k]].sum()) for k in range(st.shape[1])]          # int64 is exact: every partial sum is bounded by n < 2^63
    nz = d != 0
    out["sum_dns"] = _exact_sum(c[nz], d[nz])
    out["sum_dns2"] = _exact_sum_sq(c[nz], d[nz])
    out["T1"] = _exact_sum(c[nz], np.abs(d[nz]))
    out["T2"] = out["sum_dns2"]
    pos = d > 0
    out["sum_nodal"] = [_exact_sum(c[pos], nod[pos, b]) for b in range(nod.shape[1])]
    out["Tb"] = [_exact_sum(c[pos], np.abs(nod[pos, b])) for b in range(nod.shape[1])]
    return out


def unique_stable(states):
    """(distinct rows of states[n, ncomp] in order of first appearance, their multiplicities): nsqMain.m:220-229."""
    st = np.ascontiguousarray(np.asarray(states) != 0, dtype=np.uint8)
    if st.shape[0] == 0:
        return st, np.zeros(0, dtype=np.int64)
    packed = np.ascontiguousarray(np.packbits(st, axis=1))
    keys = packed.view(np.dtype((np.void, packed.shape[1]))).ravel()
    _, first, counts = np.unique(keys, return_index=True, return_counts=True)
    order = np.argsort(first, kind="stable")
    return st[first[order]], counts[order].astype(np.int64)


def edge_components(ncomp):
    return tuple(k for k in EDGE_BITS if k < ncomp) + (ncomp - 1,)


def dns_class(dns, fail_threshold=1e-4):
    """Name of the edge class of each dns value (DNS_CLASSES)."""
    d = np.asarray(dns, dtype=np.float64)
    out = np.empty(d.shape, dtype=object)
    out[:] = "large"
    out[d == np.nextafter(fail_threshold, 1.0)] = "above_threshold"
    out[d == fail_threshold] = "threshold"
    out[(d > 0) & (d < fail_threshold)] = "below_threshold"
    out[d < 0] = "negative"
    out[d == 0] = "zero"
    return out


def synthetic_rows(case, R, seed, max_it=150, fail_threshold=1e-4):
    """R database rows for `case` (its ncomp and nb only) with pairwise distinct outage masks and contents on every edge of the reduction:
    counts mostly small, many equal to 1, up to eight near 2^40 (sum of count * iters far below 2^63); dns exactly 0, slightly negative,
    inside (0, threshold), exactly the threshold, the next double above it, and large; nodal rows non-zero everywhere, also under the
    dns values that must keep them out of the sums; status and relaxed over 0..3, iters over 0..max_it; among the rows with dns above the
    threshold, components 0, 31, 32, 63, 64 and ncomp-1 each set in some rows and clear in others (from 36 rows on)."""
    rng = np.random.default_rng([int(seed), int(R), int(case.ncomp)])
    nc, nb = case.ncomp, case.nb
    R = int(R)
    # dns: the first rows walk through the classes (so each is present from R = 6 on, the first row being a large value), the rest are drawn
    cls = rng.choice(6, size=R, p=[0.45, 0.05, 0.05, 0.10, 0.05, 0.30])
    cls[:min(R, 36)] = np.arange(min(R, 36)) % 6
    dns = np.empty(R)
    dns[cls == 0] = rng.uniform(0.1, 3000.0, size=int((cls == 0).sum()))
    dns[cls == 1] = fail_threshold
    dns[cls == 2] = np.nextafter(fail_threshold, 1.0)
    dns[cls == 3] = rng.uniform(1e-9, 0.999 * fail_threshold, size=int((cls == 3).sum()))
    dns[cls == 4] = -rng.uniform(1e-9, 1e-6, size=int((cls == 4).sum()))
    dns[cls == 5] = 0.0
    # counts
    count = rng.integers(1, 60, size=R, dtype=np.int64)
    count[rng.random(R) < 0.25] = 1
    big = rng.choice(R, size=min(8, R // 4), replace=False)
    count[big] = (1 << 40) + rng.integers(-1000, 1000, size=big.size)
    status = rng.integers(0, 4, size=R).astype(np.int32)
    relaxed = rng.integers(0, 4, size=R).astype(np.uint8)
    iters = rng.integers(0, max_it + 1, size=R).astype(np.int32)
    if R >= 2:
        iters[0], iters[1] = max_it, 0
    nodal = rng.uniform(0.5, 100.0, size=(R, nb))
    # masks: uniform bits, then the edge bits forced on the first failing rows (set in one, clear in the next), then distinctness
    states = rng.integers(0, 2, size=(R, nc), dtype=np.uint8)
    failing = np.flatnonzero(dns > fail_threshold)

    def force(st):
        if failing.size >= 2 * len(edge_components(nc)):
            for j, k in enumerate(edge_components(nc)):
                st[failing[2 * j], k] = 1
                st[failing[2 * j + 1], k] = 0
    force(states)
    forced = set(failing[:2 * len(edge_components(nc))].tolist())
    while True:
        packed = np.ascontiguousarray(np.packbits(states, axis=1))
        keys = packed.view(np.dtype((np.void, packed.shape[1]))).ravel()
        _, first = np.unique(keys, return_index=True)
        if first.size == R:
            break
        dup = np.setdiff1d(np.arange(R), first)
        redraw = np.array([r for r in dup if r not in forced] or dup.tolist(), dtype=np.int64)
        states[redraw] = rng.integers(0, 2, size=(redraw.size, nc), dtype=np.uint8)
        force(states)
    return dict(states=states, count=count, dns=dns, nodal=nodal, status=status, iters=iters, relaxed=relaxed,
                flag=(dns > fail_threshold).astype(np.int32))


def rows_of_map(rows):
    """{packed state bytes: row index}: the database as a map from state to row."""
    packed = np.packbits(np.asarray(rows["states"]) != 0, axis=1)
    m = {}
    for r in range(packed.shape[0]):
        m[packed[r].tobytes()] = r
    assert len(m) == packed.shape[0], "a state on two rows"
    return m
