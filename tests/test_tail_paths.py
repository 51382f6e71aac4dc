"""The dynamic tail of the fused path on the 16-lane tile (csrc/relmc_kernels.hip, phase B of relmc_eval_kernel and relmc_tail_replay_kernel):
the last T scenario groups of every wavefront's range are handed out through a device counter, their fp64 contributions parked per group
and added to the owner's record afterwards in group order.  The sums must be those of the static assignment bit for bit, whichever
wavefront ran which group, so every GPU test compares the default with `static_tail` as integers and as raw fp64 bits, never with a
tolerance.  Sizes follow from the grid: W wavefronts of four-scenario groups.  The CPU test checks the plan itself (TailPlan, relmc_ctx.h)."""
import ctypes as C

import numpy as np
import pytest

from powersystemsreliabilityassessment_amd import _lib, api, case24

WPB, SPW = 4, 4          # wavefronts per workgroup and scenarios per group of the 16-lane tile


def tail_plan(n, waves):
    """(T, phase-A begin [waves], phase-A end [waves], owner [waves * T], group [waves * T]) of a launch of n scenarios (relmc_debug_tail_plan)"""
    f = _lib.load().relmc_debug_tail_plan
    cap = waves * 16
    ab, ae, ow, gr = np.full(waves, -1, np.int64), np.full(waves, -1, np.int64), np.full(cap, -1, np.int32), np.full(cap, -1, np.int64)
    t = f(n, waves, ab.ctypes.data, ae.ctypes.data, ow.ctypes.data, gr.ctypes.data)
    assert 0 <= t <= 16, t
    assert (ow[waves * t:] == -1).all() and (gr[waves * t:] == -1).all()
    return t, ab, ae, ow[:waves * t], gr[:waves * t]


def test_tail_plan_covers_every_group_once():
    """Every n from 0 to 20 000 on grids of 8, 512 and 2048 wavefronts: phase-A ranges plus tail items cover each group exactly once, the
    tail is off below 2 T groups per wavefront, a wavefront's items are its last T groups in increasing k."""
    t_on = tail_plan(1 << 24, 8)[0]
    assert t_on >= 1
    for waves in (8, 512, 2048):
        w = np.arange(waves, dtype=np.int64)
        last = None
        for n in range(0, 20001):
            ng = (n + SPW - 1) // SPW
            got = tail_plan(n, waves)
            if last is not None and last[0] == ng:          # the plan is a function of the group count: same arrays as for the n before
                assert got[0] == last[1][0] and all(np.array_equal(x, y) for x, y in zip(got[1:], last[1][1:])), n
                continue
            last = (ng, got)
            t, ab, ae, ow, gr = got
            begin, end = ng * w // waves, ng * (w + 1) // waves          # the static assignment's ranges
            assert t == (t_on if (end - begin).min() >= 2 * t_on else 0), (n, waves, t)
            assert np.array_equal(ab, begin) and np.array_equal(ae, end - t) and (ab <= ae).all(), (n, waves)
            assert ab[0] == 0 and end[-1] == ng
            if t:
                p = np.arange(waves * t)
                assert np.array_equal(ow, p % waves), (n, waves)
                assert np.array_equal(gr, end[ow] - t + p // waves), (n, waves)          # the owner's last T groups, in increasing k
                assert (gr >= ae[ow]).all() and (gr < end[ow]).all()
            if ng % 61 == 0 or ng < 64:          # and counted group by group
                cnt = np.zeros(ng + 1, np.int64)
                for lo, hi in zip(ab, ae):
                    cnt[lo:hi] += 1
                np.add.at(cnt, gr, 1)
                assert (cnt[:ng] == 1).all() and cnt[ng] == 0, (n, waves)
    assert _lib.load().relmc_debug_tail_plan(-1, 8, None, None, None, None) < 0 and _lib.load().relmc_debug_tail_plan(100, 0, None, None, None, None) < 0


# ---- GPU ------------------------------------------------------------------------------------------------------------------------

class Ctx:
    """One engine on the shipped case for the whole module, the grid's wavefront count and the plan's T"""
    eng = None
    waves = 0
    T = 0


@pytest.fixture(scope="module")
def ctx():
    c = Ctx()
    c.eng = api.Engine(case24.rts24(), device=0)
    out = (C.c_int32 * 9)()
    c.eng.L.relmc_debug_schedule.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    assert c.eng.L.relmc_debug_schedule(c.eng._h, out) == 0
    assert int(out[7]) == 2, "two workgroups per CU"
    c.waves = c.eng.tail_groups()[2]          # CUs x 2 x 4
    assert c.waves > 0 and c.waves % (2 * WPB) == 0
    c.T = tail_plan(1 << 30, c.waves)[0]
    assert c.T >= 1
    yield c
    c.eng.debug_set("static_tail", False)
    c.eng.close()


def both_tails(c, fn, expect_tail=True):
    """fn() under the static assignment and under the default (dynamic tail where the launch is large enough) of the same context"""
    c.eng.debug_set("static_tail", True)
    a = fn()
    assert c.eng.tail_groups()[0] == 0
    c.eng.debug_set("static_tail", False)
    k0 = c.eng.tail_groups()[1]
    b = fn()
    t, k1 = c.eng.tail_groups()[:2]
    if expect_tail is None:          # several launches: some of them ran with the tail
        assert k1 > k0, (k0, k1)
    elif expect_tail:
        assert t == c.T and k1 > k0, (t, k0, k1)
    else:
        assert t == 0 and k1 == k0, (t, k0, k1)
    return a, b


def assert_same_bits(a, b):
    ai, ad = a.to_arrays(); bi, bd = b.to_arrays()
    assert np.array_equal(ai, bi), np.flatnonzero(ai != bi)
    assert np.array_equal(ad.view(np.uint64), bd.view(np.uint64)), np.flatnonzero(ad.view(np.uint64) != bd.view(np.uint64))


def sizes(c):
    w, t = c.waves, c.T
    return {"2T-1": SPW * w * (2 * t - 1), "2T": SPW * w * 2 * t, "18": SPW * w * 18, "uneven": SPW * w * 2 * t + SPW * 37 + 3}


@pytest.mark.gpu
def test_tail_is_off_below_two_t_groups_per_wave(ctx):
    """2 T - 1 groups per wavefront: the launch is the static one, and the library says so (the T that RELMC_VERBOSE prints per launch)"""
    n = sizes(ctx)["2T-1"]
    assert tail_plan(n, ctx.waves)[0] == 0
    a, b = both_tails(ctx, lambda: ctx.eng.nsq_accumulate(5, 1000, n), expect_tail=False)
    assert a.n == n and a.n_fail > 0
    assert_same_bits(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("size", ["2T", "18", "uneven"])
def test_tail_gives_the_bits_of_the_static_assignment(ctx, size):
    """2 T groups per wavefront (the smallest launch with the tail on); 18 (the last window has two groups, the tail straddles two windows);
    uneven ranges with a partial last group"""
    n = sizes(ctx)[size]
    assert tail_plan(n, ctx.waves)[0] == ctx.T
    a, b = both_tails(ctx, lambda: ctx.eng.nsq_accumulate(5, 1000, n))
    assert a.n == n and a.n_fail > 0 and a.sum_dns > 0
    assert_same_bits(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("policy", [api.REFERENCE_EMULATE, api.PHYSICAL])
@pytest.mark.parametrize("seed", [1, 7, 20261016])
def test_tail_seeds_and_policies(ctx, seed, policy):
    n = sizes(ctx)["uneven"]
    a, b = both_tails(ctx, lambda: ctx.eng.nsq_accumulate(seed, 0, n, api.mpoption(policy)))
    assert a.n == n and a.n_fail > 0
    assert_same_bits(a, b)


@pytest.mark.gpu
def test_tail_is_reproducible_call_to_call(ctx):
    """The claim order is free; the bits are not"""
    n = sizes(ctx)["18"]
    ctx.eng.debug_set("static_tail", False)
    runs = [ctx.eng.nsq_accumulate(11, 123456, n) for _ in range(3)]
    assert ctx.eng.tail_groups()[0] == ctx.T
    assert_same_bits(runs[0], runs[1]); assert_same_bits(runs[0], runs[2])


@pytest.mark.gpu
def test_tail_groups_feed_the_retry_list(ctx):
    """max_it = 12 leaves the harder states non-converged: tail groups list units for the second attempt like any other group"""
    n = sizes(ctx)["18"]
    seen = []
    def limited():
        before = ctx.eng.retry_stats()
        r = ctx.eng.nsq_accumulate(3, 5000, n, api.mpoption(max_it=12))
        seen.append(tuple(int(x) - int(y) for x, y in zip(ctx.eng.retry_stats(), before)))
        return r
    a, b = both_tails(ctx, limited)
    assert seen[0][0] > 0 and seen[0] == seen[1], seen
    assert_same_bits(a, b)


@pytest.mark.gpu
def test_tail_keeps_the_checkpoint_histories(ctx):
    """nsqMain with the reference's batch of 100: stretches of many checkpoints per launch, per-sample dns written by tail groups too"""
    n = 3 * sizes(ctx)["2T"] // 100 * 100
    def run():
        return ctx.eng.nsqMain(beta_limit=0.0, max_iterations=n, samples_per_batch=100, seed=9)
    a, b = both_tails(ctx, run, expect_tail=None)
    assert a.current_iteration == b.current_iteration == n
    for h in ("beta_history", "edns_history", "lole_history", "plc_history"):
        x, y = getattr(a, h), getattr(b, h)
        assert x.size == y.size and x.size > 0 and np.array_equal(x.view(np.uint64), y.view(np.uint64)), h
    assert_same_bits(a.acc, b.acc)
