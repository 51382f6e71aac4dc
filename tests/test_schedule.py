"""The static solver schedule, checked on the CPU: `relmc_debug_symbolic` builds the pass program of a case without a device,
tests/schedule_interp.py executes it with numpy in the kernel's data layout, and the result must equal numpy.linalg.solve on the dense
bus-pair system.  Covers the elimination orders (primary + the two further orders of the retry path), every pass form, both tiles, and
random networks up to the tiles' limits.  (The reference delegates this solve to MATLAB's `\\` inside MIPS, mc_simulation.m:41.)"""
import numpy as np
import pytest

from powersystemsreliabilityassessment_amd import case24, case96
from tests import schedule_interp as si
from tests.test_random_cases import random_case


def _check(case, variant, seed, outages=0):
    s = si.symbolic(case, variant)
    rng = np.random.default_rng(seed)
    line_on = None
    if outages:
        line_on = np.ones(case.nl, bool); line_on[rng.choice(case.nl, outages, replace=False)] = False
    W, A, rhs = si.random_system(s, rng, line_on)
    x = si.solve(s, W)
    ref = np.linalg.solve(A, rhs)
    assert np.abs(x - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max()), (variant, np.abs(x - ref).max())
    return s


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_rts24_schedule_solves_the_block_system(variant):
    s = _check(case24.rts24(), variant, 1)
    assert s.tile == 0 and s.rw == 16 and s.nb == 24
    _check(case24.rts24(), variant, 2, outages=3)


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_rts96_schedule_solves_the_block_system(variant):
    s = _check(case96.rts96(), variant, 3)
    assert s.tile == 1 and s.rw == 64 and s.nb == 73
    _check(case96.rts96(), variant, 4, outages=5)


def test_schedule_sizes_do_not_regress():
    """Dependent passes per Newton step (update + inversion + back substitution): what the kernel's solver time is proportional to."""
    s24 = si.symbolic(case24.rts24()); s96 = si.symbolic(case96.rts96())
    assert s24.npass <= 21 and s96.npass <= 32


@pytest.mark.parametrize("seed,nb,chords,ng,loads", [(1, 2, 0, 2, 1), (2, 7, 3, 4, 4), (3, 19, 8, 9, 10), (4, 30, 14, 12, 14), (5, 60, 25, 30, 35),
                                                     (6, 100, 26, 40, 50), (7, 120, 6, 40, 60)])
def test_random_networks(seed, nb, chords, ng, loads):
    rng = np.random.default_rng(100 + seed)
    case = random_case(rng, nb, chords, ng, loads)
    for variant in (0, 1, 2):
        try:
            _check(case, variant, seed)
        except RuntimeError as e:                       # a further order may not fit the tile (fill, passes): then it is simply unavailable
            assert variant != 0 and "relmc_debug_symbolic failed (-4)" in str(e), e


# ---- the primary elimination order as a tunable of the schedule (relmc_tune_order / relmc_case_order_hint) ------------------------------
def _cost(s):
    nf = s.npass_upd - s.npass_updh - s.npass_updq
    lds = nf * 10 + s.npass_updh * 7 + s.npass_updq * 6 + s.npass_inv * 6 + sum(6 if (s.bwd_half >> k) & 1 else 7 for k in range(s.npass_bwd))
    return lds, s.npass


@pytest.mark.parametrize("make,seed", [(case24.rts24, 11), (case96.rts96, 12)])
def test_shipped_tuned_orders_solve_the_block_system_and_are_cheaper(make, seed):
    """The orders the package ships for RTS-24 / RTS-96 (case.elim_order): valid permutations with the reference bus last, their pass programs
    solve the bus-pair system (numpy interpreter against a dense solve, with and without line outages), and they cost fewer LDS instructions per
    Newton step than the built-in rule's order with no more dependent passes -- the reason they exist."""
    case = make()
    order = case.elim_order
    assert sorted(order.tolist()) == list(range(case.nb)) and order[-1] == case.ref_bus
    s = si.symbolic(case, 0, order)
    rule = si.symbolic(case, 0)
    assert [int(order[k]) for k in range(case.nb)] == [int(e) for e in sorted(range(case.nb), key=lambda e: s.b_int[e])]     # the hint IS the order
    (lds, npass), (lds0, npass0) = _cost(s), _cost(rule)
    assert lds < lds0 and npass <= npass0, (lds, npass, lds0, npass0)
    for outages in (0, 4):
        rng = np.random.default_rng(seed + outages)
        line_on = None
        if outages:
            line_on = np.ones(case.nl, bool); line_on[rng.choice(case.nl, outages, replace=False)] = False
        W, A, rhs = si.random_system(s, rng, line_on)
        x = si.solve(s, W)
        ref = np.linalg.solve(A, rhs)
        assert np.abs(x - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max())


def test_tune_order_is_deterministic_never_worse_and_validated():
    """relmc_tune_order on a random 30-bus network: a permutation with the reference bus last, the same for the same seed, its cost (LDS
    instructions + 4 per pass: what it minimises) never above the start's, and its schedule solves the system; relmc_debug_symbolic
    (= relmc_case_load's symbolic part) refuses hints that are not such permutations."""
    from powersystemsreliabilityassessment_amd import api
    case = random_case(np.random.default_rng(77), 30, 14, 12, 14)
    o1, st1 = api.tune_order(case, 1500, seed=5)
    o2, st2 = api.tune_order(case, 1500, seed=5)
    assert np.array_equal(o1, o2) and st1 == st2
    assert sorted(o1.tolist()) == list(range(case.nb)) and o1[-1] == case.ref_bus
    assert st1["lds_after"] + 4 * st1["passes_after"] <= st1["lds_before"] + 4 * st1["passes_before"]
    s = si.symbolic(case, 0, o1)
    assert _cost(s) == (st1["lds_after"], st1["passes_after"])
    W, A, rhs = si.random_system(s, np.random.default_rng(3))
    assert np.abs(si.solve(s, W) - np.linalg.solve(A, rhs)).max() <= 1e-9 * max(1.0, np.abs(rhs).max())
    o3, st3 = api.tune_order(case, 300, seed=6, start=o1)                 # a start order is honoured
    assert (st3["lds_before"], st3["passes_before"]) == (st1["lds_after"], st1["passes_after"])
    bad = o1.copy(); bad[0] = bad[1]
    with pytest.raises(RuntimeError, match="not a permutation"):
        si.symbolic(case, 0, bad)
    rot = np.roll(o1, 1)                                                   # the reference bus is no longer last
    with pytest.raises(RuntimeError, match="not a permutation"):
        si.symbolic(case, 0, rot)
    with pytest.raises(RuntimeError):
        si.symbolic(case, 0, o1[:-1])


def test_symbolic_images_match_their_pinned_digests():
    """Everything relmc_debug_symbolic and relmc_debug_task_image write (headers and arrays) for RTS-24 / RTS-96 under the rule's three orders
    and their shipped orders and for the random networks of this file and of tests/test_pass_shadow.py, as SHA-256 against
    tests/golden/symbolic_image_digest.json (a refused case: its return code).  Every result of the solver is a function of these bytes, so
    a refactoring of the scheduler must leave them alone; a deliberate change of the scheduler, the placement or the shadowing regenerates
    the fixture (tests/golden/make_symbolic_digest.py), and such a change owes the parity pins a run (tests/tools/order_select.py)."""
    import importlib.util
    import json
    import os
    from powersystemsreliabilityassessment_amd import _lib
    here = os.path.dirname(os.path.abspath(__file__))
    spec = importlib.util.spec_from_file_location("make_symbolic_digest", os.path.join(here, "golden", "make_symbolic_digest.py"))
    msd = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(msd)
    with open(msd.FIXTURE) as f:
        want = json.load(f)
    cases = msd.cases()
    assert [c[0] for c in cases] == list(want)
    L = _lib.load()
    got = {name: msd.digest(L, case, variant, order) for name, case, variant, order in cases}
    assert got == want, [name for name in want if got[name] != want[name]]


def test_shipped_rts24_order_is_what_the_tuner_returns():
    """Provenance of case24.RTS24_ELIM_ORDER: relmc_tune_order(60000 evaluations, seed 11) from the rule's order, bit for bit (the tuner is
    deterministic; a change of the scheduler or of its cost model shows up here, and the shipped orders are then due for a new tuning and a
    new run of tests/tools/order_select.py against the parity pins)."""
    from powersystemsreliabilityassessment_amd import api
    case = case24.rts24()
    order, st = api.tune_order(case, 60000, seed=11)
    assert (st["lds_before"], st["passes_before"], st["lds_after"], st["passes_after"]) == (174, 21, 168, 21)
    assert np.array_equal(order, case24.RTS24_ELIM_ORDER)
