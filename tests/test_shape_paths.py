"""The fused path's two evaluation kernels: the one that reads the case's shape at run time and the one with the shipped RTS-24 shape compiled
in (csrc/relmc_shape.h, relmc_shape_rts24.h).  Both run the same program on the same tables, so their results are compared as integers and
as raw fp64 bits, never with a tolerance.  The CPU test pins the checked-in header to what relmc_case_load computes for case24.rts24()."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from powersystemsreliabilityassessment_amd import _abi, _lib, api, case24

# ShapeField order of csrc/relmc_shape.h
FIELDS = ["rw", "nb", "ng", "nl", "ninj", "nzero", "off_rhs", "npass_upd", "npass_updh", "npass_updq", "npass_inv", "npass",
          "maxdeg0", "maxdeg1", "maxinj0", "maxinj1", "bwd_all_half", "stash_off", "scen_doubles"]


def shapes(case):
    """(shape relmc_case_load computes for `case` under its own elimination order, shape compiled into the specialised kernel)"""
    f = _lib.load().relmc_debug_shape
    f.restype = C.c_int32
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    holder = _abi.CaseHolder(case)
    order = getattr(case, "elim_order", None)
    o = None if order is None else np.ascontiguousarray(order, dtype=np.int32)
    got, static = np.full(64, -1, np.int32), np.full(64, -1, np.int32)
    n = f(C.byref(holder.desc), None if o is None else o.ctypes.data, 0 if o is None else int(o.size), got.ctypes.data, static.ctypes.data)
    assert n == len(FIELDS), n
    return dict(zip(FIELDS, map(int, got[:n]))), dict(zip(FIELDS, map(int, static[:n])))


def drop_line(case, k):
    """`case` without line k (the shape then differs from the shipped one in nl)"""
    keep = np.arange(case.nl) != k
    keepc = np.concatenate([np.ones(case.ng, bool), keep])
    return dataclasses.replace(case, nl=case.nl - 1, br_from=case.br_from[keep].copy(), br_to=case.br_to[keep].copy(), br_b=case.br_b[keep].copy(),
                               br_rate=case.br_rate[keep].copy(), unavail=case.unavail[keepc].copy(), always_up=case.always_up[keepc].copy())


def test_header_is_the_shape_of_the_shipped_case():
    got, static = shapes(case24.rts24())
    assert got == static, {k: (got[k], static[k]) for k in FIELDS if got[k] != static[k]}
    case = case24.rts24()
    assert (got["nb"], got["ng"], got["nl"], got["ninj"]) == (case.nb, case.ng, case.nl, case.ng + case.nd)
    # one line less is another shape: such a case must not be given the specialised kernel
    got37, _ = shapes(drop_line(case, case.nl - 1))
    assert got37["nl"] == 37 and got37 != static


def both_paths(eng, fn):
    """fn() under the specialised and under the forced run-time-shape kernel of the same context"""
    eng.debug_set("dynamic_shape", False)
    assert eng.shape_path() == "static"
    a = fn()
    eng.debug_set("dynamic_shape", True)
    assert eng.shape_path() == "dynamic"
    b = fn()
    eng.debug_set("dynamic_shape", False)
    return a, b


def assert_same_bits(a, b):
    ai, ad = a.to_arrays(); bi, bd = b.to_arrays()
    assert np.array_equal(ai, bi), np.flatnonzero(ai != bi)
    assert np.array_equal(ad.view(np.uint64), bd.view(np.uint64)), np.flatnonzero(ad.view(np.uint64) != bd.view(np.uint64))


@pytest.mark.gpu
@pytest.mark.parametrize("policy", [api.REFERENCE_EMULATE, api.PHYSICAL])
@pytest.mark.parametrize("seed", [1, 7, 20261016])
def test_static_and_dynamic_paths_give_the_same_bits(seed, policy):
    eng = api.Engine(case24.rts24(), device=0)
    try:
        a, b = both_paths(eng, lambda: eng.nsq_accumulate(seed, 0, 1_000_000, api.mpoption(policy)))
        assert a.n == 1_000_000 and a.n_fail > 0 and a.sum_dns > 0
        assert_same_bits(a, b)
    finally:
        eng.close()


@pytest.mark.gpu
def test_paths_agree_with_and_without_a_second_attempt():
    """A range every state of which converges under the primary order, and a max_it-limited run whose non-converged states go through
    the retry levels (further orders = other pass counts: always the run-time-shape kernel)."""
    eng = api.Engine(case24.rts24(), device=0)
    try:
        u0 = eng.retry_stats()[0]
        a, b = both_paths(eng, lambda: eng.nsq_accumulate(3, 5000, 200_000))
        assert eng.retry_stats()[0] == u0 and a.n_nonconverged == 0
        assert_same_bits(a, b)
        seen = []
        def limited():
            before = eng.retry_stats()[0]
            r = eng.nsq_accumulate(3, 5000, 200_000, api.mpoption(max_it=12))
            seen.append(eng.retry_stats()[0] - before)
            return r
        a, b = both_paths(eng, limited)
        assert seen[0] > 0 and seen[0] == seen[1], seen
        assert_same_bits(a, b)
    finally:
        eng.close()


@pytest.mark.gpu
def test_one_line_less_runs_the_dynamic_path_and_matches_the_oracle():
    from oracle import coracle
    case = drop_line(case24.rts24(), case24.rts24().nl - 1)
    eng = api.Engine(case, device=0)
    orc = coracle.Oracle(case)
    try:
        assert eng.shape_path() == "dynamic"
        n, seed = 4000, 11
        st = eng.mc_sampling(None, n, seed=seed, first_index=0)
        assert np.array_equal(st, orc.mc_sampling(seed, 0, n))
        for policy in (api.REFERENCE_EMULATE, api.PHYSICAL):
            dns, nodal, info = eng.mc_simulation(st, mpopt=api.mpoption(policy), return_info=True)
            ref = orc.mc_simulation(st, policy, nthreads=8)
            bad = ref["status"] != info["status"]
            assert bad.mean() < 2e-3, (bad.sum(), n)
            ok = ~bad & (ref["status"] == 0)
            np.testing.assert_allclose(dns[ok], ref["dns"][ok], rtol=0, atol=1e-5)
            dit = np.abs(info["iters"][ok] - ref["iters"][ok])
            assert dit.max() <= 2 and (dit > 1).mean() < 1e-3 and (dit > 0).mean() < 0.02
            shed = ~bad & (dns > 0)
            assert shed.sum() > 0
            np.testing.assert_allclose(nodal.sum(1)[shed & ok], dns[shed & ok], rtol=0, atol=5e-2)
        acc = eng.nsq_accumulate(seed, 100, n)
        racc = orc.nsq_accumulate(seed, 100, n)
        ai, ad = acc.to_arrays(); ri, rd = racc.to_arrays()
        assert ai[0] == n and abs(int(ai[1]) - int(ri[1])) <= 1 and np.abs(ai[6:] - ri[6:]).max() <= 1
        np.testing.assert_allclose(ad[0], rd[0], rtol=1e-6)
        assert eng.shape_path() == "dynamic"
    finally:
        eng.close()
