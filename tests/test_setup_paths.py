"""The per-scenario setup of the evaluation kernel (status -> model, island rules, block entries, start point) on the states that decide
which of its paths a row takes: the single-island path of a wavefront without a line outage, the general path beside it, every island rule,
the singular start-point path, the start point with z0 below and above 1, partial groups and windows, and the 64-lane tile.

Reference: the C oracle, under the contract of tests/test_gpu_parity.py for explicit states -- status exact, dns to 1e-6 MW, iteration
counts equal but for +-1 on fewer than 1 % of the states, integer accumulators exact (the iteration sum within that +-1 rule), fp64 sums to
1e-8.  Every state is solved by the oracle on the CPU first and none is left out of a comparison.

Which rule a state exercises follows from how it is built and is confirmed from the results: status 3 is the singular path; the oracle's
`relaxed` count marks rules 2 and 4 (an explicit-state call returns no such flag from the device; the device's own count, n_infeasible, is
compared on sampled ranges); rule 3 sheds exactly the isolated bus' load."""
import numpy as np
import pytest

from powersystemsreliabilityassessment_amd import api, case96

pytestmark = pytest.mark.gpu

DNS_TOL = 1e-6
POLICIES = [api.REFERENCE_EMULATE, api.PHYSICAL]


def _incident(case, b):
    return np.flatnonzero((case.br_from == b) | (case.br_to == b))


def _explicit_states(case):
    """(names, states[n, ncomp]) built from the case's own branch table."""
    ng, nl, nc = case.ng, case.nl, case.ncomp
    names, rows = [], []

    def add(name, comps):
        s = np.zeros(nc, dtype=np.uint8)
        s[np.asarray(comps, dtype=np.int64)] = 1
        names.append(name); rows.append(s)

    add("none", [])
    for l in range(nl):
        add(f"line{l}", [ng + l])
    for b in range(case.nb):
        add(f"iso{b}", ng + _incident(case, b))
    # one two-bus island: the end buses of the first line, cut off by every other line at either of them
    f, t = int(case.br_from[0]), int(case.br_to[0])
    cut = [l for l in np.union1d(_incident(case, f), _incident(case, t)) if {int(case.br_from[l]), int(case.br_to[l])} != {f, t}]
    add("island2", ng + np.asarray(cut))
    add("allgen", np.arange(ng))
    gb = int(case.inj_bus[0])
    add("busunits", np.flatnonzero(case.inj_bus[:ng] == gb))
    return names, np.array(rows)


@pytest.fixture(scope="module")
def explicit(case, oracle):
    names, st = _explicit_states(case)
    assert len(names) == 1 + case.nl + case.nb + 3 and case.nl == 38 and case.nb == 24
    ref = {p: oracle.mc_simulation(st, p, nthreads=8) for p in POLICIES}
    return names, st, ref


def _check(dns, info, ref):
    assert np.array_equal(info["status"], ref["status"])
    assert np.abs(dns - ref["dns"]).max() <= DNS_TOL
    dit = np.abs(info["iters"] - ref["iters"])
    assert dit.max() <= 1 and (dit > 0).sum() <= max(1, len(dit) // 100)          # fewer than 1 % of the states; one on a short list


@pytest.mark.parametrize("policy", POLICIES)
def test_explicit_states_match_oracle(engine, case, explicit, policy):
    names, st, ref = explicit
    dns, nodal, info = engine.mc_simulation(st, mpopt=api.mpoption(policy), return_info=True)
    _check(dns, info, ref[policy])
    iso = np.array([n.startswith("iso") for n in names])
    if policy == api.REFERENCE_EMULATE:
        # the singular path: every isolated bus (and nothing else of this list but the two-bus cut, whose buses keep their own line)
        assert np.all(info["status"][iso] == 3) and info["status"][names.index("none")] == 0
    else:
        assert np.all(info["status"] == 0)
        has_gen = np.bincount(case.inj_bus[:case.ng], minlength=case.nb) > 0
        rule2 = [names.index(f"iso{b}") for b in range(case.nb) if has_gen[b] and case.bus_pd[b] == 0]
        rule3 = [names.index(f"iso{b}") for b in range(case.nb) if not has_gen[b] and case.bus_pd[b] > 0]
        assert rule2 and rule3
        assert np.all(ref[policy]["relaxed"][rule2] > 0)                       # rule 2: units without load are decommitted
        assert np.all(ref[policy]["relaxed"][rule3] == 0)
        for i in rule3:                                                        # rule 3: load without generation is shed, all of it
            b = int(names[i][3:])
            assert dns[i] >= case.bus_pd[b] - 1e-5 and nodal[i, b] == pytest.approx(case.bus_pd[b], abs=2e-2)


def test_over_generation_rule_at_a_load_scale_near_zero(engine, case, oracle, explicit):
    """Rule 4 through the scaled-load entry: at a load scale near 0 the units' minimum outputs exceed the load."""
    from powersystemsreliabilityassessment_amd import seq as rseq
    names, st, _ = explicit
    pick = [names.index(k) for k in ("none", "line0", "line10", "island2", "busunits")]
    states = np.repeat(st[pick], 3, axis=0)
    scale = np.tile([1e-3, 0.05, 1.0], len(pick))
    sq = rseq.SeqEngine(engine)
    fired = 0
    for policy in POLICIES:
        ref = oracle.seq_mcsimulation(states, scale, policy, nthreads=8)
        dns, nodal, info = sq.seq_mcsimulation(states, scale, mpopt=api.mpoption(policy), return_info=True)
        _check(dns, info, ref)
        low = scale < 0.01
        fired += int((ref["relaxed"][low & (ref["status"] == 0)] > 0).sum())
        assert np.all(ref["relaxed"][(scale == 1.0) & (np.repeat(pick, 3) == pick[0])] == 0)
    assert fired > 0                                                           # rule 4 occurred (no island of these states is without load)


def test_rows_do_not_depend_on_their_wavefront(engine, explicit):
    """The same states four to a group in mixed order (rows with and without a line outage share wavefronts: the general path) and each
    state alone beside three no-outage states (a state without a line outage then takes the single-island path): bitwise equal."""
    names, st, _ = explicit
    n = len(st)
    order = np.random.default_rng(5).permutation(n)
    lout = st[:, engine.case.ng:].any(1)
    assert lout[order].reshape(-1)[: n - n % 4].reshape(-1, 4).any(1).sum() > n // 8 and (~lout).sum() >= 3
    padded = np.zeros((4 * n, st.shape[1]), dtype=np.uint8)
    padded[::4] = st
    for policy in POLICIES:
        o = api.mpoption(policy)
        d1, n1, i1 = engine.mc_simulation(st[order], mpopt=o, return_info=True)
        d2, n2, i2 = engine.mc_simulation(padded, mpopt=o, return_info=True)
        assert np.array_equal(d1.view(np.uint64), d2[::4][order].view(np.uint64))
        assert np.array_equal(i1["status"], i2["status"][::4][order]) and np.array_equal(i1["iters"], i2["iters"][::4][order])
        assert np.array_equal(n1.view(np.uint64), n2[::4][order].view(np.uint64))
        assert np.all(d2.reshape(-1, 4)[:, 1:] == 0) and np.all(i2["status"].reshape(-1, 4)[:, 1:] == 0)


@pytest.mark.parametrize("n", [1, 3, 4, 5, 63, 64, 65, 257])
def test_fused_sizes_match_oracle(engine, oracle, n):
    """Partial groups and partial windows of the fused path."""
    for policy in POLICIES:
        acc = engine.nsq_accumulate(13, 4321, n, api.mpoption(policy))
        ref = oracle.nsq_accumulate(13, 4321, n, policy)
        ai, ad = acc.to_arrays(); ri, rd = ref.to_arrays()
        assert ai[0] == n and np.array_equal(ai[:5], ri[:5]) and np.array_equal(ai[6:], ri[6:])
        assert abs(int(ai[5]) - int(ri[5])) <= n // 200
        np.testing.assert_allclose(ad[:2], rd[:2], rtol=1e-8, atol=1e-9)


def test_fused_infeasible_and_singular_counts(engine, oracle):
    """The device's own counts of the rows an island rule relaxed and of the singular rows, on a sampled range that holds both."""
    n = 20000
    for policy in POLICIES:
        acc = engine.nsq_accumulate(11, 5000, n, api.mpoption(policy))
        ref = oracle.nsq_accumulate(11, 5000, n, policy)
        assert (acc.n, acc.n_fail, acc.n_singular, acc.n_infeasible, acc.n_nonconverged) == (n, ref.n_fail, ref.n_singular, ref.n_infeasible, ref.n_nonconverged)
        assert acc.sum_dns == pytest.approx(ref.sum_dns, rel=1e-8)
        if policy == api.REFERENCE_EMULATE:
            assert acc.n_singular > 0
        else:
            assert acc.n_singular == 0


@pytest.mark.parametrize("z0", [0.5, 2.0])
def test_start_point_z0(engine, oracle, z0):
    """z0 < 1 takes the start point's divisions (mu = 1/z where that exceeds z0), z0 >= 1 does not."""
    st = engine.mc_sampling(None, 64, seed=17, first_index=900)
    for policy in POLICIES:
        o = api.mpoption(policy, z0=z0)
        ref = oracle.mc_simulation(st, policy, opts=o, nthreads=8)
        dns, _, info = engine.mc_simulation(st, mpopt=o, return_info=True)
        _check(dns, info, ref)


def test_rts96_wide_tile(case):
    """64-lane tile: no outage, 8 single line outages, 2 isolated buses."""
    from oracle import coracle
    c96 = case96.rts96()
    ng = c96.ng
    rows = [[]] + [[ng + l] for l in range(0, c96.nl, c96.nl // 8)][:8] + [list(ng + _incident(c96, b)) for b in (6, c96.nb - 1)]
    st = np.zeros((len(rows), c96.ncomp), dtype=np.uint8)
    for i, r in enumerate(rows):
        st[i, np.asarray(r, dtype=np.int64)] = 1
    assert len(rows) == 11
    orc = coracle.Oracle(c96)
    eng = api.Engine(c96, device=0)
    try:
        for policy in POLICIES:
            ref = orc.mc_simulation(st, policy, nthreads=8)
            dns, _, info = eng.mc_simulation(st, mpopt=api.mpoption(policy), return_info=True)
            _check(dns, info, ref)
            if policy == api.REFERENCE_EMULATE:
                assert np.all(info["status"][-2:] == 3) and np.all(info["status"][:-2] == 0)
    finally:
        eng.close()
