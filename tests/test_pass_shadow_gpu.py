"""Solver passes whose idle lanes shadow an active lane (csrc/relmc_dev.h, "idle lanes"), on the device.

Small random networks leave most lanes of every pass idle, so nearly every lane of these runs computes on shadowed operands and must
store nothing: the explicit-state entry point (MODE 1) against the C oracle, and one fused launch that stops after three iterations,
where rows of a wavefront end while others go on, against the run-time-shape kernel of the same context as raw bits.
"""
import numpy as np
import pytest

from powersystemsreliabilityassessment_amd import api, case24
from tests.test_random_cases import random_case

pytestmark = pytest.mark.gpu

DNS_TOL = 1e-6          # tests/test_gpu_parity.py


def _case(name):
    if name == "rts24":
        return case24.rts24()
    seed, nb, chords, ng, loads = {"nb5": (8, 5, 2, 3, 3), "nb9": (9, 9, 3, 4, 4)}[name]
    return random_case(np.random.default_rng(100 + seed), nb, chords, ng, loads)


@pytest.mark.parametrize("name", ["nb5", "nb9", "rts24"])
def test_explicit_states_match_the_oracle(name):
    from oracle import coracle
    case = _case(name)
    eng = api.Engine(case, device=0)
    try:
        orc = coracle.Oracle(case)
        st = eng.mc_sampling(None, 256, seed=1, first_index=0)
        assert np.array_equal(st, orc.mc_sampling(1, 0, 256))
        dns, nodal, info = eng.mc_simulation(st, mpopt=api.mpoption(api.REFERENCE_EMULATE), return_info=True)
        ref = orc.mc_simulation(st, api.REFERENCE_EMULATE, nthreads=8)
        print(name, "status differs on", int((info["status"] != ref["status"]).sum()), "iterations differ on", int((info["iters"] != ref["iters"]).sum()),
              "max |dns - ref|", float(np.abs(dns - ref["dns"]).max()))
        assert np.array_equal(info["status"], ref["status"])
        assert np.array_equal(info["iters"], ref["iters"])
        np.testing.assert_allclose(dns, ref["dns"], rtol=0, atol=DNS_TOL)
    finally:
        eng.close()


def test_fused_launch_cut_short_gives_the_bits_of_the_run_time_shape_kernel():
    eng = api.Engine(case24.rts24(), device=0)
    try:
        res = []
        for dynamic in (False, True):
            eng.debug_set("dynamic_shape", dynamic)
            assert eng.shape_path() == ("dynamic" if dynamic else "static")
            res.append(eng.nsq_accumulate(5, 1000, 4096, api.mpoption(max_it=3)))
        eng.debug_set("dynamic_shape", False)
        (ai, ad), (bi, bd) = res[0].to_arrays(), res[1].to_arrays()
        assert ai[0] == 4096
        assert np.array_equal(ai, bi)
        assert np.array_equal(ad.view(np.uint64), bd.view(np.uint64))
    finally:
        eng.close()
