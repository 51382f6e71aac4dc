"""CPU side of tests/test_db_edges.py: the plain database model (tests/tools/db_model.py) is tied to the oracle's own restatement of the
reference's loop, its row generator is shown to contain every edge it promises, and the sampled ranges of the probe-overflow test are shown
to overflow the probe kernel's block table.  No GPU."""
import dataclasses
import importlib.util
import os

import numpy as np
import pytest

from powersystemsreliabilityassessment_amd import _abi, case24, case96

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


dbm = _tool("db_model")

# the probe-overflow test (test_db_edges.py imports these): seed, first sample index, number of samples; block table and window of the probe kernel
OVERFLOW_SEED, OVERFLOW_FIRST, OVERFLOW_N = 20240611, 123_456_789, 8192 + 37
PROBE_WINDOW, PROBE_SLOTS = 1024, 512


def high_outage(case):
    """`case` with an unavailability of 0.5 on every component that can fail: practically every sample is a state of its own."""
    return dataclasses.replace(case, unavail=np.where(np.asarray(case.always_up) != 0, case.unavail, 0.5))


@pytest.mark.parametrize("policy", [_abi.RELMC_REFERENCE_EMULATE, _abi.RELMC_PHYSICAL])
def test_model_accumulate_is_the_oracles_accumulation(oracle, policy):
    """accumulate(rows of the oracle's database) = the accumulators the oracle's own loop over those rows gives: integers exactly, doubles to the
    rounding of the oracle's summation.  The oracle adds R products one after the other in fp64: one rounding for count * dns (two for
    count * dns * dns) and R - 1 additions, a chain of at most R + 1 roundings, so its sum lies within (R + 1) * 2^-53 * T * (1 + O(R 2^-53)) of
    the exact one, T the sum of the magnitudes of the terms; the model's own error (<= 2^-53 * T, the final rounding) is one more.  Bound used:
    2 * (R + 2) * 2^-53 * T."""
    ref = oracle.nsq_database(seed=6, beta_limit=0.0, max_iterations=4000, samples_per_batch=100, policy=policy, max_rows=4000)
    R = len(ref["count"])
    assert 100 < R < 4000 and ref["count"].sum() == 4000
    got = dbm.accumulate(ref)
    acc = ref["acc"]
    for k in ("n", "n_fail", "n_singular", "n_nonconverged", "n_infeasible", "n_screened", "sum_iters"):
        assert got[k] == getattr(acc, k), k
    assert got["n_fail"] > 0 and got["sum_iters"] > 0
    assert got["comp_fail"] == list(acc.comp_fail)[:oracle.case.ncomp] and not any(list(acc.comp_fail)[oracle.case.ncomp:])
    u = 2.0 ** -53
    assert abs(acc.sum_dns - got["sum_dns"]) <= 2 * (R + 2) * u * got["T1"]
    assert abs(acc.sum_dns2 - got["sum_dns2"]) <= 2 * (R + 2) * u * got["T2"]
    for b in range(oracle.case.nb):
        assert abs(acc.sum_nodal[b] - got["sum_nodal"][b]) <= 2 * (R + 2) * u * got["Tb"][b], b
    assert got["sum_dns"] > 0 and max(got["sum_nodal"]) > 0


def test_unique_stable_is_the_oracles_dedupe(oracle):
    """unique_stable(sampled states) = the states and count columns of the oracle's database over the same samples (one batch and many)."""
    n = 3000
    st = oracle.mc_sampling(6, 0, n)
    u, c = dbm.unique_stable(st)
    for batch in (100, n):
        ref = oracle.nsq_database(seed=6, beta_limit=0.0, max_iterations=n, samples_per_batch=batch, max_rows=n)
        assert np.array_equal(u, ref["states"]) and np.array_equal(c, ref["count"])
    assert c.sum() == n and c.max() > 1 and len(c) < n
    # by hand
    u, c = dbm.unique_stable(np.array([[0, 1], [1, 1], [0, 1], [0, 0], [1, 1], [0, 1]]))
    assert u.tolist() == [[0, 1], [1, 1], [0, 0]] and c.tolist() == [3, 2, 1]
    u, c = dbm.unique_stable(np.zeros((0, 5), dtype=np.uint8))
    assert u.shape == (0, 5) and c.shape == (0,)


def test_model_accumulate_by_hand():
    """Each comparison of the model on rows small enough to sum by hand."""
    rows = dict(states=np.array([[1, 0, 1], [0, 1, 1], [1, 1, 0], [0, 0, 1], [0, 0, 0]]), count=np.array([2, 3, 5, 7, 11]),
                dns=np.array([1e-4, np.nextafter(1e-4, 1.0), 2.0, -0.5, 0.0]), nodal=np.array([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0], [7.0, 8.0], [9.0, 10.0]]),
                status=np.array([0, 1, 2, 3, 3]), iters=np.array([1, 2, 3, 4, 5]), relaxed=np.array([0, 1, 2, 3, 0]))
    a = dbm.accumulate(rows)
    assert (a["n"], a["n_fail"], a["n_singular"], a["n_nonconverged"], a["n_infeasible"], a["n_screened"]) == (28, 8, 18, 8, 10, 12)
    assert a["sum_iters"] == 2 + 6 + 15 + 28 + 55 and a["comp_fail"] == [5, 8, 3]
    assert a["sum_dns"] == pytest.approx(2e-4 + 3e-4 + 10.0 - 3.5, rel=1e-15) and a["T1"] == pytest.approx(2e-4 + 3e-4 + 10.0 + 3.5, rel=1e-15)
    assert a["sum_dns2"] == pytest.approx(5e-8 + 20.0 + 1.75, rel=1e-15)
    assert a["sum_nodal"] == [2 * 1.0 + 3 * 3.0 + 5 * 5.0, 2 * 2.0 + 3 * 4.0 + 5 * 6.0]


@pytest.mark.parametrize("which,R", [("rts24", 257), ("rts24", 65537), ("rts96", 257), ("rts96", 65537)])
def test_synthetic_rows_contain_every_edge(which, R):
    case = case24.rts24() if which == "rts24" else case96.rts96()
    rows = dbm.synthetic_rows(case, R, seed=11)
    st, c, d, nod = rows["states"], rows["count"], rows["dns"], rows["nodal"]
    assert st.shape == (R, case.ncomp) and nod.shape == (R, case.nb) and set(np.unique(st)) == {0, 1}
    assert len(np.unique(np.packbits(st, axis=1), axis=0)) == R                                    # pairwise distinct masks
    # counts
    assert c.min() == 1 and (c == 1).sum() >= R // 8 and np.median(c) < 64 and c.max() < 2 ** 53
    assert 4 <= ((c > 2 ** 40 - 2000) & (c < 2 ** 40 + 2000)).sum() <= 8
    assert sum(int(a) * int(b) for a, b in zip(c.tolist(), rows["iters"].tolist())) < 2 ** 63
    # dns classes
    cls = dbm.dns_class(d)
    for name in dbm.DNS_CLASSES:
        assert (cls == name).sum() >= 4, name
    assert np.all(d[cls == "threshold"] == 1e-4) and np.all(d[cls == "above_threshold"] == np.nextafter(1e-4, 1.0))
    assert np.all((d[cls == "below_threshold"] > 0) & (d[cls == "below_threshold"] < 1e-4)) and np.all(d[cls == "negative"] < 0)
    assert d[cls == "large"].min() > 1e-4 and d.max() > 1000
    assert np.array_equal(rows["flag"], (d > 1e-4).astype(np.int32))
    # nodal rows: non-zero everywhere, in particular where the device must leave them out
    assert np.all(nod != 0) and (d <= 0).sum() >= 8
    # status / relaxed / iters
    assert set(np.unique(rows["status"])) == {0, 1, 2, 3} and set(np.unique(rows["relaxed"])) == {0, 1, 2, 3}
    assert rows["iters"].min() == 0 and rows["iters"].max() == 150
    # mask bits among the failing rows
    f = d > 1e-4
    comps = dbm.edge_components(case.ncomp)
    assert comps == (0, 31, 32, 63, 64, case.ncomp - 1)
    for k in comps:
        assert 0 < st[f, k].sum() < f.sum(), k
    # the same seed gives the same rows, another seed others
    again = dbm.synthetic_rows(case, R, seed=11)
    assert all(np.array_equal(rows[k], again[k]) for k in rows)
    assert not np.array_equal(dbm.synthetic_rows(case, R, seed=12)["states"], st)


def test_synthetic_rows_small_counts():
    case = case24.rts24()
    for R in (1, 2, 255, 256):
        rows = dbm.synthetic_rows(case, R, seed=3)
        assert len(np.unique(np.packbits(rows["states"], axis=1), axis=0)) == R == len(rows["count"])
    assert dbm.synthetic_rows(case, 1, seed=3)["dns"][0] > 1e-4            # the one-row database is a failing row, not a trivial one


@pytest.mark.parametrize("which", ["rts24", "rts96"])
def test_probe_overflow_condition(which):
    """Condition of test_db_edges.py's probe-overflow test, not a measurement: with the committed seed, first index and length, every full
    1024-sample window of the range (counted from its start: the probe kernel's block b takes samples [1024 b, 1024 b + 1024)) holds at least
    513 distinct states, one more than the kernel's block table has slots, so every such window must take the direct-atomic fallback.  The range
    ends with a partial window of 37 samples (it cannot overflow anything; it is there for the kernel's bound check)."""
    case = high_outage(case24.rts24() if which == "rts24" else case96.rts96())
    from oracle import coracle
    st = coracle.Oracle(case).mc_sampling(OVERFLOW_SEED, OVERFLOW_FIRST, OVERFLOW_N)
    assert not st[:, np.asarray(case.always_up) != 0].any()
    full = OVERFLOW_N // PROBE_WINDOW
    assert full == 8 and OVERFLOW_N % PROBE_WINDOW == 37
    for w in range(full):
        u, _ = dbm.unique_stable(st[w * PROBE_WINDOW:(w + 1) * PROBE_WINDOW])
        assert len(u) >= PROBE_SLOTS + 1, (w, len(u))
