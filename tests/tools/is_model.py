"""Host model of the importance-sampling track (relmc_is_ratios, relmc_is_sampling, relmc_nsq_is_accumulate, relmc_nsq_is_indices,
relmc_nsq_is_tune; contract in include/relmc.h) in NumPy: oracle.pyoracle's Philox draws against the tilted thresholds, the likelihood
ratios from the integer thresholds, the ascending product, the weighted sums and estimators, and the cross-entropy update rule.
Shared by tests/test_importance_host.py (no GPU) and tests/test_importance.py (device against this model)."""
import math

import numpy as np

from oracle import pyoracle

TWO32 = 4294967296.0
FAIL = 1e-4                                             # nsqMain.m:270


def thresholds(unavail, always_up=None):
    """relmc_case_load's rule: floor(u * 2^32), at most 2^32 - 1, 0 where always_up."""
    u = np.asarray(unavail, dtype=np.float64)
    t = np.minimum(np.floor(u * TWO32), 4294967295.0)
    t = np.where(t > 0, t, 0.0)
    if always_up is not None:
        t = np.where(np.asarray(always_up) != 0, 0.0, t)
    return t.astype(np.uint32)


def tilt_thresholds(thr, always_up, unavail_is):
    """thr_is of a tilt, or ValueError naming the first offending component (the refusals of relmc_is_ratios)."""
    thr = np.asarray(thr, dtype=np.uint32)
    if unavail_is is None:
        return thr.copy()
    q = np.asarray(unavail_is, dtype=np.float64)
    au = np.zeros(thr.size, dtype=np.uint8) if always_up is None else np.asarray(always_up)
    out = np.zeros(thr.size, dtype=np.uint32)
    for k in range(thr.size):                           # component by component: the first offence is the one reported
        if not (np.isfinite(q[k]) and 0.0 <= q[k] <= 1.0):
            raise ValueError(f"component {k}: not a number in [0, 1]")
        out[k] = thresholds(q[k:k + 1], au[k:k + 1])[0]
        if out[k] == 0 and thr[k] > 0:
            raise ValueError(f"component {k}: the tilted law does not cover the nominal one")
    return out


def ratios(thr, thr_is):
    """(r_dn, r_up): one fp64 division of exactly representable integers each; r_dn = 1.0 where thr_is == 0."""
    t, s = np.asarray(thr, dtype=np.float64), np.asarray(thr_is, dtype=np.float64)
    r_dn = np.ones(t.size)
    nz = s > 0
    r_dn[nz] = t[nz] / s[nz]
    return r_dn, (TWO32 - t) / (TWO32 - s)


def weights(states, r_dn, r_up):
    """W[i] = product over k ascending of r_dn[k] (down) / r_up[k] (up), from 1.0, one rounded multiply per component."""
    st = np.asarray(states) != 0
    W = np.ones(st.shape[0])
    for k in range(st.shape[1]):
        W = W * np.where(st[:, k], r_dn[k], r_up[k])
    return W


def sample(thr, thr_is, seed, first_index, n):
    """(states [n, ncomp] uint8, W [n]) of samples [first_index, first_index + n): relmc_mc_sampling's draws against thr_is."""
    st = pyoracle.mc_sampling(thr_is, seed, first_index, n)
    return st, weights(st, *ratios(thr, thr_is))


def state_probability(thr, x):
    """P(x) under the integer thresholds thr (exact rationals in fp64 up to the product's rounding)."""
    p = np.asarray(thr, dtype=np.float64) / TWO32
    return float(np.prod(np.where(np.asarray(x) != 0, p, 1.0 - p)))


def accumulate(states, W, dns, nodal=None, status=None, iters=None):
    """relmc_is_acc's fields from per-sample outputs (math.fsum: the correctly rounded sums the device's fixed-order sums are compared with)."""
    st = np.asarray(states) != 0
    W, dns = np.asarray(W, dtype=np.float64), np.asarray(dns, dtype=np.float64)
    fail = dns > FAIL
    wf, wd = np.where(fail, W, 0.0), W * dns
    col = lambda f, M: np.array([math.fsum(f * M[:, k]) for k in range(M.shape[1])])
    acc = dict(n=int(W.size), n_fail=int(fail.sum()),
               sum_w=math.fsum(W), sum_w2=math.fsum(W * W), sum_wfail=math.fsum(wf), sum_w2fail=math.fsum(np.where(fail, W * W, 0.0)),
               sum_wdns=math.fsum(wd), sum_w2dns2=math.fsum(wd * wd),
               comp_wfail=col(wf, st.astype(np.float64)), comp_wdns=col(wd, st.astype(np.float64)))
    if nodal is not None:
        acc["sum_wnodal"] = col(W, np.asarray(nodal, dtype=np.float64))
    if status is not None:
        s = np.asarray(status)
        acc["n_singular"], acc["n_nonconverged"] = int((s == 3).sum()), int(((s == 1) | (s == 2)).sum())
    if iters is not None:
        acc["sum_iters"] = int(np.asarray(iters, dtype=np.int64).sum())
    return acc


def beta_of(s, s2, n):
    """relmc_nsq_indices' beta from a sum and a sum of squares."""
    mean = s / n
    ss = max(s2 - n * mean * mean, 0.0)
    return math.sqrt(ss) / n / mean if mean > 0 else math.inf


def indices(acc, hours=8760.0):
    """relmc_nsq_is_indices from a dict of relmc_is_acc's fields."""
    n = float(acc["n"])
    edns, plc = acc["sum_wdns"] / n, acc["sum_wfail"] / n
    out = dict(n=acc["n"], edns=edns, plc=plc, lole=plc * hours, eens=edns * hours,
               beta=beta_of(acc["sum_wdns"], acc["sum_w2dns2"], n), beta_plc=beta_of(acc["sum_wfail"], acc["sum_w2fail"], n),
               mean_w=acc["sum_w"] / n, ess=acc["sum_w"] ** 2 / acc["sum_w2"] if acc["sum_w2"] > 0 else 0.0,
               mean_iters=acc.get("sum_iters", 0) / n,
               comp_importance=np.asarray(acc["comp_wfail"]) / acc["sum_wfail"] if acc["sum_wfail"] > 0 else np.zeros(len(acc["comp_wfail"])))
    if "sum_wnodal" in acc:
        out["nodal_eens"] = np.asarray(acc["sum_wnodal"]) / n
    return out


def shortfall(case, states):
    """m_i = total_load - sum over the in-service real generators, ascending, of max(inj_pmax, 0)."""
    st = np.asarray(states) != 0
    cap = np.zeros(st.shape[0])
    for g in range(case.ng):
        cap = cap + np.where(st[:, g], 0.0, max(float(case.inj_pmax[g]), 0.0))
    return case.total_load - cap


def elite_weights(case, states, W, dns, min_elite=100, rho=0.1, objective=1):
    """One pass's elites: (e [n], final, level).  Final pass (|F| >= min_elite): e = W (objective 0) or W dns (1) on F.  Level pass: F plus
    the ceil(rho n) - |F| non-failed samples of largest shortfall (ties: the lower index), e = W; level = the smallest shortfall added."""
    W, dns = np.asarray(W, dtype=np.float64), np.asarray(dns, dtype=np.float64)
    fail = dns > FAIL
    nf, n = int(fail.sum()), W.size
    if nf >= min_elite:
        return np.where(fail, W * dns if objective == 1 else W, 0.0), True, math.nan
    e = np.where(fail, W, 0.0)
    add = min(max(int(math.ceil(rho * n)) - nf, 0), n - nf)
    level = math.nan
    if add > 0:
        m = shortfall(case, states)
        rest = np.flatnonzero(~fail)
        pick = rest[np.argsort(-m[rest], kind="stable")[:add]]
        e[pick] = W[pick]
        level = float(m[pick[-1]])
    return e, False, level


def ce_update(q, p, always_up, states, e, alpha=1.0, q_max=0.5):
    """q_k <- max(min(alpha v_k + (1 - alpha) q_k, q_max), p_k), 0 where always_up; v_k = sum e_i x_ik / sum e_i (sum e_i in sample order)."""
    se = 0.0
    for x in np.asarray(e, dtype=np.float64):
        se += x
    if not se > 0.0:
        return np.array(q, dtype=np.float64)
    st = (np.asarray(states) != 0).astype(np.float64)
    v = np.array([math.fsum(e * st[:, k]) for k in range(st.shape[1])]) / se
    x = np.maximum(np.minimum(alpha * v + (1.0 - alpha) * np.asarray(q, dtype=np.float64), q_max), p)
    return np.where(np.asarray(always_up) != 0, 0.0, x)


def tune(case, evaluate, seed=1, n_pilot=20000, max_iters=5, final_iters=2, min_elite=100, rho=0.1, objective=1, alpha=1.0, q_max=0.5):
    """relmc_nsq_is_tune with `evaluate(states) -> dns` in the place of the device.  Returns (q, report): report = list of dicts per pass."""
    thr = thresholds(case.unavail, case.always_up)
    p = thr.astype(np.float64) / TWO32
    q, report, finals = p.copy(), [], 0
    for t in range(max_iters):
        if finals >= final_iters:
            break
        st, W = sample(thr, tilt_thresholds(thr, case.always_up, q), seed, t * n_pilot, n_pilot)
        dns = np.asarray(evaluate(st), dtype=np.float64)
        e, final, level = elite_weights(case, st, W, dns, min_elite, rho, objective)
        finals += int(final)
        report.append(dict(n_fail=int((dns > FAIL).sum()), n_elite=int((e > 0).sum()), sum_e=float(sum(e.tolist())), final=final, level=level))
        q = ce_update(q, p, case.always_up, st, e, alpha, q_max)
    return q, report
