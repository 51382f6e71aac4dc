"""The two forms of an interior-point trip's front half (csrc/relmc_kernels.hip, kNormSplitMask): with the four second-stage termination
norms, taken when the first stage of the convergence test holds for some row of the wavefront, and without them.  The diagnosis switch
`norms_always` makes every trip take the form with the norms, which is what every trip did before the split.  Both must give the same
verdicts on the same trips, so every comparison here is of raw bytes between the default and `norms_always`, toggled back and forth on
one Engine, never with a tolerance."""
import json
import os

import numpy as np
import pytest

from powersystemsreliabilityassessment_amd import api, case24, case96, seq

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def eng24():
    eng = api.Engine(case24.rts24(), device=0)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def eng96():
    eng = api.Engine(case96.rts96(), device=0)
    yield eng
    eng.close()


def both_forms(eng, fn):
    """fn() under the default, under norms_always, and under the default again"""
    eng.debug_set("norms_always", False)
    a = fn()
    eng.debug_set("norms_always", True)
    b = fn()
    eng.debug_set("norms_always", False)
    c = fn()
    return a, b, c


def raw(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint8).reshape(-1)


def assert_same_acc(a, b):
    ai, ad = a.to_arrays(); bi, bd = b.to_arrays()
    assert np.array_equal(ai, bi), np.flatnonzero(ai != bi)
    assert np.array_equal(raw(ad), raw(bd)), np.flatnonzero(ad.view(np.uint64) != bd.view(np.uint64))


def assert_same_states(r0, r1):
    (d0, n0, i0), (d1, n1, i1) = r0, r1
    assert np.array_equal(i0["status"], i1["status"]), np.flatnonzero(i0["status"] != i1["status"])
    assert np.array_equal(i0["iters"], i1["iters"]), np.flatnonzero(i0["iters"] != i1["iters"])
    assert np.array_equal(raw(d0), raw(d1)), np.flatnonzero(d0.view(np.uint64) != d1.view(np.uint64))
    assert np.array_equal(raw(n0), raw(n1))


def states_of(name, ncomp):
    with open(os.path.join(GOLDEN, name)) as f:
        d = json.load(f)
    st = np.zeros((len(d["states"]), ncomp), dtype=np.uint8)
    for i, x in enumerate(d["states"]):
        st[i, x["failed"]] = 1
    return d["states"], st


# ---- 1. fused path, RTS-24 ----------------------------------------------------------------------------------------------------------
N_FUSED = 8192 + 3          # the last group of four is partial


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["default", "static_tail", "dynamic_shape"])
@pytest.mark.parametrize("policy", [api.REFERENCE_EMULATE, api.PHYSICAL])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_fused_path_gives_the_same_acc(eng24, seed, policy, variant):
    if variant != "default":
        eng24.debug_set(variant, True)
    try:
        assert eng24.shape_path() == ("dynamic" if variant == "dynamic_shape" else "static")
        a, b, c = both_forms(eng24, lambda: eng24.nsq_accumulate(seed, 0, N_FUSED, api.mpoption(policy)))
    finally:
        if variant != "default":
            eng24.debug_set(variant, False)
    assert a.n == N_FUSED and a.sum_iters >= 12 * (N_FUSED - a.n_singular) and a.n_fail > 0 and a.sum_dns > 0
    assert_same_acc(a, b)
    assert_same_acc(a, c)


@pytest.mark.gpu
def test_fused_path_with_the_dynamic_tail_gives_the_same_acc(eng24):
    """A launch long enough for the dynamic tail to be on (the 8 195-scenario launches above are too short for it), so that groups claimed
    through the tail counter run both forms too."""
    n = 400_003
    a, b, c = both_forms(eng24, lambda: eng24.nsq_accumulate(1, 0, n))
    assert a.n == n and eng24.tail_groups()[0] > 0
    assert_same_acc(a, b)
    assert_same_acc(a, c)


# ---- 2. per-scenario outputs on explicit states --------------------------------------------------------------------------------------
def mixed_states24():
    """Fixture states ordered so that every group of four (one wavefront) holds 12-iteration states beside 14-15-iteration ones: its rows pass
    the first stage on different trips.  The all-up state, G24 + G33 out, the singular states and the slowest states (16-21) are in."""
    recs, st = states_of("states_fixture.json", case24.rts24().ncomp)
    it = np.array([x["emulate"]["iters"] for x in recs]); status = np.array([x["emulate"]["status"] for x in recs])
    failed = [x["failed"] for x in recs]
    all_up, g24_g33 = failed.index([]), failed.index([23, 32])
    assert it[all_up] == 12 and it[g24_g33] == 14
    fast = [i for i in np.flatnonzero((status == 0) & (it <= 12)) if i != all_up]
    slow = [i for i in np.flatnonzero((status == 0) & (it >= 14)) if i != g24_g33]
    other = list(np.flatnonzero(status == 3)) + list(np.flatnonzero((status == 0) & (it == 13)))
    order = [all_up, g24_g33, fast.pop(), slow.pop()]
    while slow and len(fast) >= 2:          # {12, 14+, 12, 14+ or singular / 13}
        order += [fast.pop(), slow.pop(), fast.pop(), other.pop() if other else slow.pop() if slow else fast.pop()]
    order = np.array(order)
    groups = it[order][:len(order) // 4 * 4].reshape(-1, 4)
    assert ((groups <= 12).any(1) & (groups >= 14).any(1)).all()
    assert (status[order] == 3).sum() == (status == 3).sum() > 0 and it[order].max() == it.max()
    return st[order], it[order], status[order]


@pytest.mark.gpu
@pytest.mark.parametrize("policy", [api.REFERENCE_EMULATE, api.PHYSICAL])
def test_explicit_states_mixed_in_every_group(eng24, policy):
    st, it, status = mixed_states24()
    r = both_forms(eng24, lambda: eng24.mc_simulation(st, mpopt=api.mpoption(policy), return_info=True))
    assert_same_states(r[0], r[1])
    assert_same_states(r[0], r[2])
    if policy == api.REFERENCE_EMULATE:          # the recorded oracle counts (the suite's parity tests allow the device +-1 on a few states)
        assert np.array_equal(r[0][2]["status"], status)
        assert np.abs(r[0][2]["iters"] - it)[status == 0].max() <= 2


@pytest.mark.gpu
def test_numerically_failed_fixture_rts96(eng96):
    """The RTS-96 states on which the primary order ends numerically failed (the failure test stays evaluated on every trip of both forms):
    first attempt and retries run the evaluation kernel of the wide tile."""
    _, st = states_of("rts96_numfail_fixture.json", case96.rts96().ncomp)
    u0 = eng96.retry_stats()[0]
    r = both_forms(eng96, lambda: eng96.mc_simulation(st, return_info=True))
    assert eng96.retry_stats()[0] - u0 == 3 * st.shape[0]          # every state failed its first attempt, under either form
    assert_same_states(r[0], r[1])
    assert_same_states(r[0], r[2])


# ---- 3. option edges -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("max_it", [1, 2, 11, 12])
def test_rows_stopped_on_or_before_their_converging_trip(eng24, max_it):
    st, it, status = mixed_states24()
    o = api.mpoption(max_it=max_it)
    r = both_forms(eng24, lambda: eng24.mc_simulation(st, mpopt=o, return_info=True))
    assert_same_states(r[0], r[1])
    assert_same_states(r[0], r[2])
    a, b, c = both_forms(eng24, lambda: eng24.nsq_accumulate(2, 0, N_FUSED, o))
    if max_it < 12:
        assert a.n_nonconverged > 0
    assert_same_acc(a, b)
    assert_same_acc(a, c)


@pytest.mark.gpu
@pytest.mark.parametrize("feastol", [1e-13, 0.0])
def test_first_stage_passes_for_many_trips_before_the_second(eng24, feastol):
    """comptol = costtol = 1e-2 lets the first stage pass early, so the form with the norms runs from then on, trip after trip.  Measured:
    feastol = 1e-13 does not hold the second stage back (the constraints are linear: a full Newton step meets them to rounding), the rows
    converge on trips 5-11; with feastol = 0 the second stage never passes and no row converges (max_it, or the failure test once gamma
    underflows)."""
    st, it, status = mixed_states24()
    o = api.mpoption(comptol=1e-2, costtol=1e-2, feastol=feastol, max_it=30)
    r = both_forms(eng24, lambda: eng24.mc_simulation(st, mpopt=o, return_info=True))
    assert_same_states(r[0], r[1])
    assert_same_states(r[0], r[2])
    nonsing = r[0][2]["status"] != 3
    if feastol == 0.0:
        assert (r[0][2]["status"][nonsing] != 0).all()
    else:
        a, b, c = both_forms(eng24, lambda: eng24.nsq_accumulate(3, 0, N_FUSED, o))
        assert a.n_nonconverged == 0
        assert_same_acc(a, b)
        assert_same_acc(a, c)


# ---- 4. other tracks -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_sequential_track_three_years(eng24):
    se = seq.SeqEngine(eng24)
    r = both_forms(eng24, lambda: se.seq_years(1, 0, 3))
    assert r[0][3].sum() > 0          # contingency hours were evaluated
    for other in (r[1], r[2]):
        for k in range(4):            # ens, dlc, nlc, n_contingency per year
            assert np.array_equal(raw(r[0][k]), raw(other[k])), k
        assert_same_acc(r[0][4], other[4])


@pytest.mark.gpu
def test_rts96_fused_path(eng96):
    n = 1024
    a, b, c = both_forms(eng96, lambda: eng96.nsq_accumulate(1, 0, n))
    assert a.n == n
    assert_same_acc(a, b)
    assert_same_acc(a, c)
    ia, ib = eng96.indices(a), eng96.indices(b)
    assert (ia.edns, ia.lole, ia.plc) == (ib.edns, ib.lole, ib.plc)
