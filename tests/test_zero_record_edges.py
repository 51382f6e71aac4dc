"""The all-zero line record nl and injection entry ninj of the evaluation (csrc/relmc_kernels.hip, kZeroBySlot): the slot lane that stands
behind the last line / injection writes them inside the evaluation's own stores, and lane 0 writes them only on a tile filled to the last
slot, where no such lane exists.  The shapes at which that can go wrong: one element short of a full tile and exactly full, for the lines and
the injections of the 16-lane tile (48 lines, 64 injections) and the injections of the 64-lane tile (192), each side of the two tests
independently; and networks of one and two lines, where almost every lane of a row is a lane beyond the last element.  Device against the
C oracle on sampled states, both policies, with the assertions of tests/test_random_cases.py::test_random_case_matches_oracle."""
import numpy as np
import pytest

from powersystemsreliabilityassessment_amd import api
from tests import schedule_interp as si
from tests.test_random_cases import random_case

pytestmark = pytest.mark.gpu

N_STATES = 1000

# (id, generator seed, nb, chords, generators, load buses, rating tightness, parallel circuits, pmin fraction, nl, ninj, lanes per scenario)
EDGES = [
    ("nl47_ninj63", 2000, 32, 16, 33, 30, 0.5, 0, 0.0, 47, 63, 16),          # a lane behind the last line and one behind the last injection
    ("nl48_ninj64", 2000, 32, 15, 34, 30, 0.5, 2, 0.0, 48, 64, 16),          # neither: lane 0 writes both dummies
    ("nl47_ninj64", 2001, 32, 14, 34, 30, 0.5, 2, 0.0, 47, 64, 16),          # the line record by a slot lane, the injection entry by lane 0
    ("nl48_ninj63", 2000, 32, 17, 33, 30, 0.5, 0, 0.0, 48, 63, 16),          # ... and the other way round
    ("wide_ninj191", 2000, 100, 20, 131, 60, 0.5, 2, 0.0, 121, 191, 64),
    ("wide_ninj192", 2000, 100, 20, 132, 60, 0.5, 2, 0.0, 121, 192, 64),
    ("one_line", 1001, 2, 0, 2, 1, 1.0, 0, 0.0, 1, 3, 16),                   # CASES[0] of test_random_cases.py without its second circuit
    ("two_lines", 1001, 2, 0, 2, 1, 1.0, 1, 0.0, 2, 3, 16),                  # CASES[0]: two buses, a double circuit
]


@pytest.mark.parametrize("spec", EDGES, ids=lambda s: s[0])
def test_edge_shape_matches_oracle(spec):
    from oracle import coracle
    _, seed, nb, chords, ng, lbs, tight, par, pminf, nl, ninj, lanes = spec
    case = random_case(np.random.default_rng(seed), nb, chords, ng, lbs, tight, par, pminf)
    assert case.nl == nl and case.ng + case.nd == ninj
    assert si.symbolic(case, 0, None).rw == lanes          # the tile relmc_case_load chose
    eng = api.Engine(case, device=0)
    orc = coracle.Oracle(case)
    try:
        n = N_STATES
        st = eng.mc_sampling(None, n, seed=seed, first_index=0)
        assert np.array_equal(st, orc.mc_sampling(seed, 0, n))
        for policy in (api.REFERENCE_EMULATE, api.PHYSICAL):
            dns, nodal, info = eng.mc_simulation(st, mpopt=api.mpoption(policy), return_info=True)
            ref = orc.mc_simulation(st, policy, nthreads=8)
            bad = ref["status"] != info["status"]
            dit = np.abs(info["iters"] - ref["iters"])[~bad & (ref["status"] == 0)]
            print("%s policy %d: status differs on %d of %d, max |dns - oracle| %.3g, iterations differ on %d (by more than one on %d), %d states shed"
                  % (spec[0], policy, bad.sum(), n, np.abs(dns - ref["dns"])[~bad & (ref["status"] == 0)].max(), (dit > 0).sum(), (dit > 1).sum(),
                     (~bad & (dns > 0)).sum()))
            assert bad.mean() < 2e-3, (bad.sum(), n)
            ok = ~bad & (ref["status"] == 0)
            np.testing.assert_allclose(dns[ok], ref["dns"][ok], rtol=0, atol=1e-5)
            assert dit.max() <= 2 and (dit > 1).mean() < 1e-3 and (dit > 0).mean() < 0.02
            shed = ~bad & (dns > 0)
            assert shed.sum() > 0                                       # the case does shed load in some states
            np.testing.assert_allclose(nodal.sum(1)[shed & ok], dns[shed & ok], rtol=0, atol=5e-2)
        acc = eng.nsq_accumulate(seed, 100, n)
        racc = orc.nsq_accumulate(seed, 100, n)
        ai, ad = acc.to_arrays(); ri, rd = racc.to_arrays()
        assert ai[0] == n and abs(int(ai[1]) - int(ri[1])) <= 1 and np.abs(ai[6:] - ri[6:]).max() <= 1
        np.testing.assert_allclose(ad[0], rd[0], rtol=1e-6)
    finally:
        eng.close()
