"""The unique-state database's own kernels (relmc_database.hip, relmc_db_kernels.h) on rows the solver never produces and at the edges of their
contracts: relmc_db_import puts rows with any keys, counts, dns, meta and nodal values on the device, the device's sums are compared with the
exact arithmetic of tests/tools/db_model.py.  Covers the chunk switch of the reduction, its four comparisons on dns and its mask-bit scatter,
the probe kernel's block table at both extremes, lookup / insert / rehash against a shuffled import, 64-bit sample indices on the HL2 paths,
the export's arguments and the import's input checks.  tests/test_db_edges_host.py ties the model to the oracle and proves the condition of the
probe-overflow test on the CPU."""
import dataclasses
import functools
import importlib.util
import os

import numpy as np
import pytest

from powersystemsreliabilityassessment_amd import api, case24, case96

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, *path, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


dbm = _load(("tests", "tools"), "db_model")
host = _load(("tests",), "test_db_edges_host")         # the committed seed / first index / length of the probe-overflow test and its case

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
FIRST_CAP = 1 << 16                                    # rows the database's arrays hold before they first double


# ---------------------------------------------------------------------------------------------- fixtures
@pytest.fixture(scope="module")
def case96_():
    return case96.rts96()


def _engine(c):
    eng = api.Engine(c, device=0)
    try:
        yield eng
    finally:
        eng.close()


@pytest.fixture(scope="module")
def engine96(case96_):
    yield from _engine(case96_)


@pytest.fixture(scope="module")
def engine_hi24(case):
    yield from _engine(host.high_outage(case))


@pytest.fixture(scope="module")
def engine_hi96(case96_):
    yield from _engine(host.high_outage(case96_))


@pytest.fixture(scope="module")
def engine_allup(case):
    yield from _engine(dataclasses.replace(case, unavail=np.zeros_like(case.unavail)))


@functools.lru_cache(maxsize=2)
def _rows(which, R):
    return dbm.synthetic_rows(case24.rts24() if which == "rts24" else case96.rts96(), R, seed=20240611)


# ---------------------------------------------------------------------------------------------- helpers
def chunking(R):
    """(rows per block, blocks) of the reduction for R rows: 256-row chunks up to 4096 blocks, then ceil(R / 4096) rows per block."""
    per, nblk = 256, -(-R // 256)
    if nblk > 4096:
        per = -(-R // 4096)
        nblk = -(-R // per)
    return per, nblk


def rounding_chain(R):
    """k: the longest chain of fp64 roundings between a row's term and sum_dns / sum_dns2 of an R-row database: ceil(per / 256) fused
    multiply-adds per thread, one more for the c * d product of sum_dns2, 8 levels of the block's tree, up to 64 lane-strided adds of block
    partials and 6 butterfly steps in the final kernel.  The nodal sums run ceil(per / 8) fused multiply-adds per thread and a 3-level tree
    instead (per <= 512 for every row count here: at most 64 + 3 + 70 = 137 roundings), which the bound 2 k u T, k >= 80, covers as well."""
    per, _ = chunking(R)
    return -(-per // 256) + 1 + 8 + 64 + 6


def expected_ints(model, ncomp):
    ints = np.zeros(api._abi.Acc.N_INT, dtype=np.int64)
    ints[:6] = [model[k] for k in ("n", "n_fail", "n_singular", "n_infeasible", "n_nonconverged", "sum_iters")]
    ints[6:6 + ncomp] = model["comp_fail"]
    ints[6 + 256] = model["n_screened"]
    return ints


def check_acc(acc, model, R, ncomp, nb, what):
    """Every integer word equal to the model's; sum_dns, sum_dns2 and every sum_nodal[b] within 2 k 2^-53 T.  Returns the worst error / tolerance."""
    ints, dbls = acc.to_arrays()
    want = expected_ints(model, ncomp)
    bad = np.flatnonzero(ints != want)
    assert bad.size == 0, (what, "integer words", bad[:8], ints[bad[:8]], want[bad[:8]])
    k = rounding_chain(R)
    terms = [("sum_dns", dbls[0], model["sum_dns"], model["T1"]), ("sum_dns2", dbls[1], model["sum_dns2"], model["T2"])]
    terms += [(f"sum_nodal[{b}]", dbls[2 + b], model["sum_nodal"][b], model["Tb"][b]) for b in range(nb)]
    worst = 0.0
    for name, got, ref, T in terms:
        tol = 2 * k * U * T
        err = abs(float(got) - ref)
        assert err <= tol, (what, name, got, ref, err, tol)
        if tol > 0:
            worst = max(worst, err / tol)
    assert not np.any(dbls[2 + nb:]), (what, "sum_nodal beyond the case's buses")
    print(f"[db_edges] {what}: R = {R}, per = {chunking(R)[0]}, blocks = {chunking(R)[1]}, k = {k}, worst error / tolerance = {worst:.3e}")
    return worst


def same_rows(a, b, keys=("states", "count", "dns", "flag", "nodal", "status", "iters", "relaxed"), sl=slice(None)):
    """Bit for bit (doubles compared as their 64-bit patterns: -0.0, the value next to the threshold)."""
    for k in keys:
        x, y = np.ascontiguousarray(np.asarray(a[k])[sl]), np.ascontiguousarray(np.asarray(b[k]))
        assert x.shape == y.shape, (k, x.shape, y.shape)
        if x.dtype == np.float64 or y.dtype == np.float64:
            assert np.array_equal(x.astype(np.float64).view(np.int64), y.astype(np.float64).view(np.int64)), k
        else:
            assert np.array_equal(x.astype(np.int64), y.astype(np.int64)), k


def take(rows, sel):
    return {k: np.asarray(v)[sel] for k, v in rows.items()}


# ---------------------------------------------------------------------------------------------- a. the reduction against the model
BIG = 1_300_003          # per = 318: a multiple of neither 256 nor 318


@pytest.mark.parametrize("which,R", [("rts24", r) for r in (1, 255, 256, 257, FIRST_CAP, FIRST_CAP + 1, 4096 * 256, 4096 * 256 + 1, BIG)] +
                         [("rts96", r) for r in (1, 257, FIRST_CAP + 1)])
def test_reduction_of_imported_rows_is_the_models(engine, engine96, which, R):
    """reset, import of synthetic rows, accumulate: the device's sums over rows that sit on every comparison of relmc_db_reduce_kernel (dns on
    the failure threshold, next to it, negative, zero with a non-zero nodal row), with counts near 2^40 and mask bits on the word and chunk
    borders, at the row counts around the 256-row chunks, the first capacity and the switch to ceil(rows / 4096) rows per block."""
    eng = engine if which == "rts24" else engine96
    rows = _rows(which, R)
    per, nblk = chunking(R)
    if R == 4096 * 256:
        assert (per, nblk) == (256, 4096)
    if R == 4096 * 256 + 1:
        assert (per, nblk) == (257, 4081)
    if R == BIG:
        assert per == 318 and R % 256 != 0 and R % per != 0 and nblk == 4089
    model = dbm.accumulate(rows)
    o = api.mpoption()
    eng.db_reset()
    try:
        eng.db_import(rows, o)
        assert eng.db_size() == (R, model["n"])
        acc = eng.db_accumulate()
        check_acc(acc, model, R, eng.case.ncomp, eng.case.nb, f"{which} reduction")
        assert bytes(eng.db_accumulate()) == bytes(acc)                    # a fixed summation order: the same bytes every time
        eng.db_reset()
        assert eng.db_size() == (0, 0) and eng.db_accumulate().n == 0
        eng.db_import(rows, o)
        assert bytes(eng.db_accumulate()) == bytes(acc) and eng.db_size() == (R, model["n"])
    finally:
        eng.db_reset()


def test_export_of_the_largest_row_set_and_its_arguments(engine):
    """Export of the 1.3e6 imported rows bit for bit (flag = dns > 1e-4 on rows on and next to the threshold), sub-ranges at the ends and across
    the first capacity, and the argument errors, after which the database still answers."""
    rows, R = _rows("rts24", BIG), BIG
    engine.db_reset()
    try:
        engine.db_import(rows, api.mpoption())
        acc = engine.db_accumulate()
        got = engine.db_export()
        same_rows(rows, got)
        assert np.array_equal(got["flag"], (rows["dns"] > 1e-4).astype(np.int32)) and 0 < got["flag"].sum() < R
        thr = rows["dns"] == 1e-4
        assert thr.sum() > 1000 and not got["flag"][thr].any() and got["flag"][rows["dns"] == np.nextafter(1e-4, 1.0)].all()
        for first, n in ((0, 0), (R, 0), (R - 1, 1), (0, 1), (FIRST_CAP - 6, 12), (4096 * 256 - 3, 7)):
            part = engine.db_export(first, n)
            assert len(part["count"]) == n
            same_rows(rows, part, sl=slice(first, first + n))
        assert len(engine.db_export(R - 5)["count"]) == 5                   # n_rows = None: to the end
        for first, n in ((0, R + 1), (R, 1), (R - 1, 2), (R + 1, 0), (-1, 1), (-1, 0), (0, -1), (R, -1)):
            with pytest.raises(api.RelmcError, match="row range"):
                engine.db_export(first, n)
        # a sum of the two arguments that does not fit 64 bits (no buffers: the call must refuse before it touches any)
        for first, n in ((2 ** 63 - 1, 1), (1, 2 ** 63 - 1), (2 ** 62, 2 ** 62)):
            assert engine.L.relmc_db_export(engine._h, first, n, None, None, None, None, None, None, None, None) == -1, (first, n)      # RELMC_ERR_INVALID
        assert engine.db_size() == (R, int(rows["count"].sum()))
        assert bytes(engine.db_accumulate()) == bytes(acc)
        same_rows(rows, engine.db_export(R - 1, 1), sl=slice(R - 1, R))
    finally:
        engine.db_reset()


# ---------------------------------------------------------------------------------------------- b. probe kernel: more distinct hits than LDS slots
@pytest.mark.parametrize("which", ["rts24", "rts96"])
def test_probe_with_more_distinct_rows_per_window_than_block_table_slots(engine_hi24, engine_hi96, which):
    """Every sample of the batch is a hit, and every full 1024-sample window holds more than 512 distinct rows (test_probe_overflow_condition
    proves that for this seed, first index and length on the CPU): the rows that find the block's table full go to memory by the direct
    64-bit atomic.  A lost or doubled increment shows in the counts, which must double exactly."""
    eng = engine_hi24 if which == "rts24" else engine_hi96
    seed, first, N = host.OVERFLOW_SEED, host.OVERFLOW_FIRST, host.OVERFLOW_N
    from oracle import coracle
    st = eng.mc_sampling(None, N, seed=seed, first_index=first)
    assert np.array_equal(st, coracle.Oracle(eng.case).mc_sampling(seed, first, N))          # the range the CPU test looked at
    u, c = dbm.unique_stable(st)
    R = len(c)
    assert R > 8 * 513 and c.sum() == N
    rows = dict(dbm.synthetic_rows(eng.case, R, seed=7))
    rows["states"], rows["count"] = u, c
    o = api.mpoption()
    eng.db_reset()
    try:
        eng.db_import(rows, o)
        acc, st_ = eng.nsq_db_batch(seed, first, N, o)
        assert (st_.new_rows, st_.rows, st_.samples, st_.batch_distinct) == (0, R, 2 * N, 0)
        assert eng.db_size() == (R, 2 * N)
        got = eng.db_export()
        doubled = dict(rows, count=2 * c)
        same_rows(doubled, got, keys=("states", "count", "dns", "nodal", "status", "iters", "relaxed"))
        check_acc(acc, dbm.accumulate(doubled), R, eng.case.ncomp, eng.case.nb, f"{which} probe overflow")
        assert bytes(eng.db_accumulate()) == bytes(acc)
    finally:
        eng.db_reset()


# ---------------------------------------------------------------------------------------------- c. probe kernel: every sample one row
def test_probe_with_a_million_samples_on_one_row(engine_allup):
    """The other extreme of the block table: no component can fail, the database has one row, and 1 000 003 further samples all land in one
    slot's counter of every block."""
    eng, seed, n0, n1 = engine_allup, 5, 100, 1_000_003
    assert not eng.thresholds().any()
    eng.db_reset()
    try:
        _, s0 = eng.nsq_db_batch(seed, 0, n0)
        assert (s0.rows, s0.new_rows, s0.samples) == (1, 1, n0)
        acc, s1 = eng.nsq_db_batch(seed, n0, n1)
        assert (s1.rows, s1.new_rows, s1.samples, s1.batch_distinct) == (1, 0, n0 + n1, 0)
        db = eng.db_export()
        assert db["count"].tolist() == [n0 + n1] and not db["states"].any() and db["dns"][0] == 0.0
        assert acc.n == n0 + n1 and acc.n_fail == 0 and acc.sum_dns == 0.0
    finally:
        eng.db_reset()


# ---------------------------------------------------------------------------------------------- d. hits and misses against a shuffled database
def _check_map(got, imported, full, n_imp):
    """The database after one batch over the range of `full` on top of `imported` rows, as a map from state to row."""
    fmap, gmap, imap = dbm.rows_of_map(full), dbm.rows_of_map(got), dbm.rows_of_map(imported)
    assert set(gmap) == set(fmap) | set(imap)
    # imported rows: where they were, keys and results untouched, counts grown by the multiplicity of their state in the range
    head = take(got, slice(0, n_imp))
    same_rows(imported, head, keys=("states", "dns", "nodal", "status", "iters", "relaxed"))
    ipacked = np.packbits(np.asarray(imported["states"]) != 0, axis=1)
    mult = np.array([full["count"][fmap[k]] if k in fmap else 0 for k in (ipacked[r].tobytes() for r in range(n_imp))], dtype=np.int64)
    assert np.array_equal(head["count"], np.asarray(imported["count"]) + mult)
    # appended rows: exactly the states of the range the import did not hold, in order of first appearance (= their order in `full`),
    # with their multiplicities and the results of the first run, bit for bit
    fpacked = np.packbits(np.asarray(full["states"]) != 0, axis=1)
    missing = np.array([r for r in range(len(full["count"])) if fpacked[r].tobytes() not in imap], dtype=np.int64)
    tail = take(got, slice(n_imp, None))
    same_rows(take(full, missing), tail, keys=("states", "count", "dns", "flag", "nodal", "status"))
    return len(missing)


def test_hits_and_misses_against_a_shuffled_import(engine):
    """Lookup, insert and the per-sample probe on a database whose row order is not the sample order: a random half of a real run's rows,
    shuffled, counts 1, then one batch over the whole range."""
    seed, n, o = 12, 200_000, api.mpoption()
    engine.db_reset()
    try:
        acc_full, _ = engine.nsq_db_batch(seed, 0, n, o)
        full = engine.db_export()
        Rf = len(full["count"])
        assert Rf > 2000 and full["count"].sum() == n
        rng = np.random.default_rng(99)
        sel = rng.permutation(Rf)[:Rf // 2]
        imported = take(full, sel)
        imported["count"] = np.ones(len(sel), dtype=np.int64)
        engine.db_reset()
        engine.db_import(imported, o)
        acc, st = engine.nsq_db_batch(seed, 0, n, o)
        got = engine.db_export()
        n_missing = _check_map(got, imported, full, len(sel))
        assert n_missing == Rf - len(sel) == st.new_rows and st.rows == Rf and st.samples == n + len(sel)
        check_acc(acc, dbm.accumulate(got), Rf, engine.case.ncomp, engine.case.nb, "shuffled import")
        assert acc.n == acc_full.n + len(sel)
    finally:
        engine.db_reset()


def test_growth_with_a_shuffled_import_in_the_table(engine):
    """65 000 imported rows (half of a real run's rows among synthetic ones, shuffled) in arrays of 65 536; the batch adds more than 536 new
    rows, so the arrays double and the table of row ids is rebuilt over the shuffled rows."""
    seed, n, o, n_imp = 12, 200_000, api.mpoption(), 65_000
    engine.db_reset()
    try:
        engine.nsq_db_batch(seed, 0, n, o)
        full = engine.db_export()
        Rf = len(full["count"])
        rng = np.random.default_rng(100)
        sel = rng.permutation(Rf)[:Rf // 2]
        assert Rf - len(sel) > FIRST_CAP - n_imp
        fmap = dbm.rows_of_map(full)
        synth = dbm.synthetic_rows(engine.case, n_imp, seed=8)
        fresh = np.array([np.packbits(synth["states"][r]).tobytes() not in fmap for r in range(n_imp)])
        synth = take(synth, np.flatnonzero(fresh)[:n_imp - len(sel)])
        real = take(full, sel)
        real["count"] = np.ones(len(sel), dtype=np.int64)
        real["relaxed"] = real["relaxed"].astype(np.uint8)
        order = rng.permutation(n_imp)
        imported = {k: np.concatenate([np.asarray(real[k]), np.asarray(synth[k]).astype(np.asarray(real[k]).dtype)])[order] for k in real}
        assert len(imported["count"]) == n_imp
        engine.db_reset()
        engine.db_import(imported, o)
        acc, st = engine.nsq_db_batch(seed, 0, n, o)
        assert st.rows == n_imp + Rf - len(sel) > FIRST_CAP and st.new_rows == Rf - len(sel) > FIRST_CAP - n_imp
        got = engine.db_export()
        assert _check_map(got, imported, full, n_imp) == st.new_rows
        check_acc(acc, dbm.accumulate(got), st.rows, engine.case.ncomp, engine.case.nb, "growth over a shuffled import")
        # the rebuilt table finds every row: a second pass over the range only bumps counts
        _, st2 = engine.nsq_db_batch(seed, 0, n, o)
        assert st2.new_rows == 0 and st2.rows == st.rows
        again = engine.db_export()
        same_rows(got, again, keys=("states", "dns", "nodal", "status", "iters", "relaxed"))
        gmap = dbm.rows_of_map(got)
        bump = np.zeros(st.rows, dtype=np.int64)
        for k, r in fmap.items():
            bump[gmap[k]] = full["count"][r]
        assert np.array_equal(again["count"], got["count"] + bump)
    finally:
        engine.db_reset()


# ---------------------------------------------------------------------------------------------- e. 64-bit sample indices on the HL2 paths
@pytest.mark.parametrize("first", [2 ** 32 - 3000, 2 ** 63 - 3000])
@pytest.mark.parametrize("which", ["rts24", "rts96"])
def test_sample_indices_across_2_32_and_2_63(engine, engine96, oracle, which, first):
    """The sampler, relmc_memo_keys_kernel and relmc_db_probe_kernel with the sample counter's upper word in use and changing inside the range."""
    from oracle import coracle
    eng = engine if which == "rts24" else engine96
    orc = oracle if which == "rts24" else coracle.Oracle(eng.case)
    seed, n, o = 21, 6000, api.mpoption()
    want = orc.mc_sampling(seed, first, n)
    assert np.array_equal(eng.mc_sampling(None, n, seed=seed, first_index=first), want)
    assert not np.array_equal(want[3000:], orc.mc_sampling(seed, 0, 3000))                   # the upper word of the index matters
    u, c = dbm.unique_stable(want)
    plain = eng.nsq_accumulate(seed, first, n, o)
    dist, nd = eng.nsq_accumulate_distinct(seed, first, n, o)
    eng.db_reset()
    try:
        acc, st = eng.nsq_db_batch(seed, first, n, o)
        one = eng.db_export()
        pi = plain.to_arrays()[0]
        assert pi[0] == n and np.array_equal(dist.to_arrays()[0], pi) and np.array_equal(acc.to_arrays()[0], pi)
        assert nd == len(c) == st.rows == st.new_rows and st.samples == n
        assert np.array_equal(one["states"], u) and np.array_equal(one["count"], c)
        # the same range in two calls: the second one probes per sample, with the boundary inside it
        eng.db_reset()
        eng.nsq_db_batch(seed, first, 2999, o)
        acc2, st2 = eng.nsq_db_batch(seed, first + 2999, n - 2999, o)
        two = eng.db_export()
        same_rows(one, two)
        assert bytes(acc2) == bytes(acc) and (st2.rows, st2.samples) == (st.rows, n)
    finally:
        eng.db_reset()


# ---------------------------------------------------------------------------------------------- f. import validation
def test_import_refuses_duplicate_states_and_iters_out_of_range(engine):
    """One row per state and iters in [0, 2^23): anything else is refused with the row named, the database stays empty and takes a valid import."""
    rows = dbm.synthetic_rows(engine.case, 300, seed=5)
    o = api.mpoption()
    engine.db_reset()
    try:
        dup = {k: v.copy() for k, v in rows.items()}
        dup["states"][211] = dup["states"][17]
        with pytest.raises(api.RelmcError, match=r"row 211 repeats the state of row 17"):
            engine.db_import(dup, o)
        assert engine.db_size() == (0, 0) and engine.db_accumulate().n == 0
        for bad, row in ((-1, 42), (2 ** 23, 299), (-2 ** 31, 0), (2 ** 31 - 1, 7)):
            b = {k: v.copy() for k, v in rows.items()}
            b["iters"][row] = bad
            with pytest.raises(api.RelmcError, match=rf"row {row} has iters = {bad}\b"):
                engine.db_import(b, o)
            assert engine.db_size() == (0, 0)
        ok = {k: v.copy() for k, v in rows.items()}
        ok["iters"][3] = 2 ** 23 - 1                                           # the largest value the row's meta word holds
        engine.db_import(ok, o)
        assert engine.db_size() == (300, int(rows["count"].sum()))
        same_rows(ok, engine.db_export())
        check_acc(engine.db_accumulate(), dbm.accumulate(ok), 300, engine.case.ncomp, engine.case.nb, "import after refusals")
    finally:
        engine.db_reset()
