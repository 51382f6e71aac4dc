"""Every HL2 entry point drives relmc_eval_kernel through one launch protocol (csrc/relmc_retry.hip: eval_collect, fail_retry and the
RetryOut accessor).  On the small case only the fused path ever sees more than a handful of listed units, so the protocol
is exercised here under a heavy load in every path: RTS-24 with an iteration limit of 7, seed 5, samples [0, 3000) -- the inputs of
test_gpu_parity.py::test_dense_last_resort_in_the_retry_chain, where more than 1000 units end non-converged, all three retry levels run
and the list (4096 entries at least) does not overflow."""
import ctypes as C

import numpy as np
import pytest

from powersystemsreliabilityassessment_amd import api

SEED, FIRST, N = 5, 0, 3000
ACCUMULATING = ("nsq_accumulate", "nsq_accumulate_distinct", "nsq_db_batch")


def retry_heavy_calls(engine):
    """The calls of the test on one engine.  Returns (results by path, counter movements by path); a movement is how far the call moved
    (retry_stats()[0], retry_dense_stats()[0], retry_overflow()).  Paths: the three accumulating ones, screen off and on ("+screen"),
    mc_simulation on host buffers ("host") and on device buffers ("dev") over the sampled states: (dns, nodal, status, iters)."""
    res, moved = {}, {}

    def call(name, f):
        m0 = (engine.retry_stats()[0], engine.retry_dense_stats()[0], engine.retry_overflow())
        res[name] = f()
        m1 = (engine.retry_stats()[0], engine.retry_dense_stats()[0], engine.retry_overflow())
        moved[name] = tuple(b - a for a, b in zip(m0, m1))

    for screen in (0, 1):
        o = api.mpoption(api.REFERENCE_EMULATE, screen=screen); o.max_it = 7
        tag = "+screen" if screen else ""
        call("nsq_accumulate" + tag, lambda: engine.nsq_accumulate(SEED, FIRST, N, o))
        call("nsq_accumulate_distinct" + tag, lambda: engine.nsq_accumulate_distinct(SEED, FIRST, N, o)[0])
        engine.db_reset()
        call("nsq_db_batch" + tag, lambda: engine.nsq_db_batch(SEED, FIRST, N, o)[0])
        engine.db_reset()
    o = api.mpoption(api.REFERENCE_EMULATE); o.max_it = 7
    st = np.ascontiguousarray(engine.mc_sampling(None, N, seed=SEED, first_index=FIRST), dtype=np.uint8)
    res["states"] = st

    def host():
        dns, nodal, info = engine.mc_simulation(st, mpopt=o, return_info=True)
        return dns, nodal, info["status"], info["iters"]

    def dev():
        # device buffers from the HIP runtime the library itself is linked against (found through the library's handle)
        hip = engine.L
        for f, args in ((hip.hipMalloc, [C.POINTER(C.c_void_p), C.c_size_t]), (hip.hipMemcpy, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]), (hip.hipFree, [C.c_void_p])):
            f.argtypes, f.restype = args, C.c_int
        out = (np.zeros(N), np.zeros((N, engine.case.nb)), np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.int32))
        ptr = []
        try:
            for a in (st,) + out:
                p = C.c_void_p()
                assert hip.hipMalloc(C.byref(p), a.nbytes) == 0
                ptr.append(p)
                assert hip.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0           # hipMemcpyHostToDevice
            assert hip.hipDeviceSynchronize() == 0                                  # the uploads are in place before the library's stream starts
            engine.mc_simulation_dev(ptr[0].value, N, *(p.value for p in ptr[1:]), mpopt=o)
            for a, p in zip(out, ptr[1:]):
                assert hip.hipMemcpy(a.ctypes.data, p, a.nbytes, 2) == 0           # hipMemcpyDeviceToHost
        finally:
            for p in ptr:
                hip.hipFree(p)
        return out

    call("host", host)
    call("dev", dev)
    return res, moved


@pytest.mark.gpu
def test_retry_heavy_in_every_path(engine):
    res, moved = retry_heavy_calls(engine)
    for name, m in moved.items():
        print("   %-32s retry units %+d, dense units %+d, overflow %+d" % (name, *m))
    for tag in ("", "+screen"):
        print("   integers%s:" % tag, [res[p + tag].to_arrays()[0][:6].tolist() for p in ACCUMULATING])
    # the integer accumulators of the three accumulating paths are one another's, screen off and, separately, on
    for tag in ("", "+screen"):
        ai = res["nsq_accumulate" + tag].to_arrays()[0]
        for p in ACCUMULATING[1:]:
            assert np.array_equal(res[p + tag].to_arrays()[0], ai), p + tag
    # screen off they are the counts of the per-state outputs, through host buffers and through device buffers
    acc = res["nsq_accumulate"]
    assert acc.n == N and acc.n_nonconverged > 1000
    for p in ("host", "dev"):
        dns, nodal, status, iters = res[p]
        assert acc.n_fail == int((dns > 1e-4).sum()), p
        assert acc.n_nonconverged == int(((status == 1) | (status == 2)).sum()), p
        assert acc.sum_iters == int(iters.sum()), p
    # every path: what went to the further orders went on to the dense solve (nothing converges within 7 iterations under any order), and
    # all of it had room on the list
    for name, (units, dense, overflow) in moved.items():
        assert units == dense > 0 and overflow == 0, (name, units, dense, overflow)
    # a unit is a sample in the fused and the per-state paths, a distinct state in the other two
    status = res["host"][2]
    bad = (status == 1) | (status == 2)
    distinct_bad = len(np.unique(res["states"][bad], axis=0))
    assert moved["nsq_accumulate"][0] == moved["host"][0] == moved["dev"][0] == acc.n_nonconverged
    assert moved["nsq_accumulate_distinct"][0] == moved["nsq_db_batch"][0] == distinct_bad
    assert moved["nsq_accumulate+screen"][0] == res["nsq_accumulate+screen"].n_nonconverged
    assert moved["nsq_accumulate_distinct+screen"][0] == moved["nsq_db_batch+screen"][0]
