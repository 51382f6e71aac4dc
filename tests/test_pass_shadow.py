"""Idle lanes of the solver passes shadow an active lane (csrc/relmc_dev.h, "idle lanes"), checked on the CPU.

`relmc_debug_task_image` exports the pass descriptors exactly as the device gets them: byte offsets, every lane without a task carrying
the read operands of an active lane of its pass plus the form's idle marker.  The tests check the image against `relmc_debug_symbolic`'s
pass program (which keeps exporting idle lanes as 0xffff) and execute it with numpy the way a shadowing kernel does -- ALL lanes load
and compute, only non-idle lanes store -- against tests/schedule_interp.py's run of the same Newton system, as raw bits.
"""
import ctypes as C

import numpy as np
import pytest

from powersystemsreliabilityassessment_amd import _abi, _lib, case24, case96
from tests import schedule_interp as si
from tests.test_random_cases import random_case

IDLE_INV = 0xffff
# ds_read_b128 serves a wavefront in four fixed groups of 16 lanes (the placement model's conflict domain, csrc/relmc_schedule.hip): lane -> group.
# On the 16-lane tile lane = 16 * scenario row + slot, and the slots {0-3, 12-15} / {4-11} share their groups in every scenario row.
READ_GROUP = [0,0,0,0,1,1,1,1,1,1,1,1,0,0,0,0, 1,1,1,1,0,0,0,0,0,0,0,0,1,1,1,1,
              2,2,2,2,3,3,3,3,3,3,3,3,2,2,2,2, 3,3,3,3,2,2,2,2,2,2,2,2,3,3,3,3]


def task_image(case, order_variant=0, order=None):
    L = _lib.load()
    hint = None if order is None else np.ascontiguousarray(order, dtype=np.int32)
    holder = _abi.CaseHolder(case)
    hdr = np.zeros(16, np.int32)
    tasks = np.zeros(96 * 64 * 4, np.uint16)
    err = C.create_string_buffer(512)
    rc = L.relmc_debug_task_image(C.byref(holder.desc), order_variant, None if hint is None else hint.ctypes.data, 0 if hint is None else int(hint.size),
                                  hdr.ctypes.data, tasks.ctypes.data, tasks.size, err, 512)
    if rc != 0:
        raise RuntimeError(f"relmc_debug_task_image failed ({rc}): {err.value.decode()}")
    h = [int(x) for x in hdr]
    rw, npass = h[1], h[5]
    return dict(tile=h[0], rw=rw, nb=h[2], nws=h[3], off_rhs=h[4], npass=npass, npass_upd=h[6], npass_inv=h[7], npass_updh=h[8], npass_updq=h[9],
                bwd_half=(h[10] & 0xffffffff) | ((h[11] & 0xffffffff) << 32), scen_doubles=h[12], cost_masked=h[13], cost_shadow=h[14], cost_tasks=h[15],
                tasks=tasks[: npass * rw * 4].reshape(npass, rw, 4).astype(np.int64))


def form_of(im, p):
    npu, npi = im["npass_upd"], im["npass_inv"]
    npuh = npu - im["npass_updq"]; npuf = npuh - im["npass_updh"]
    if p < npuf: return "full"
    if p < npuh: return "half"
    if p < npu: return "quarter"
    if p < npu + npi: return "inv"
    return "bwd_half" if (im["bwd_half"] >> (p - npu - npi)) & 1 else "bwd"


def is_idle(form, d):
    return (d[2] | d[3]) != 0 if form == "inv" else d[0] == d[3]


# reads of a lane per form: (field, byte offset behind it, bytes, alignment of the field)
READS = {
    "full": [(3, 0, 32, 16), (1, 0, 32, 16), (2, 0, 32, 16), (0, 0, 32, 16)],
    "half": [(3, 0, 32, 16), (1, 0, 16, 16), (2, 0, 32, 16), (0, 0, 16, 16)],
    "quarter": [(3, 0, 32, 16), (1, 0, 16, 16), (2, 0, 16, 16), (0, 0, 8, 8)],
    "inv": [(0, 0, 32, 16), (1, 0, 16, 16)],
    "bwd": [(1, 0, 32, 16), (2, 0, 32, 16), (3, 0, 16, 16), (0, 0, 16, 16)],
    "bwd_half": [(1, 0, 32, 16), (2, 0, 16, 16), (3, 0, 16, 16), (0, 0, 8, 8)],
}
READ_ONLY_FIELDS = {"inv": (0, 1)}          # every other form: fields 1, 2, 3 (field 0 is the target and holds the marker)


def _inv(D):
    pm, pb, pe = D[0], D[1], -D[3]
    q = 1.0 / (pm * pe + pb * pb)
    return pe * q, pb * q, -pm * q


def run_image(im, W, shadow):
    """The pass program of the device image on W (in place of a copy): with `shadow` every lane of a pass loads and computes and only the
    non-idle lanes store; without it idle lanes skip the pass.  The arithmetic is schedule_interp.solve's, expression for expression."""
    W = W.copy()
    with np.errstate(all="ignore"):
        for p in range(im["npass"]):
            form = form_of(im, p)
            stores = []
            for r in range(im["rw"]):
                d = [int(x) for x in im["tasks"][p, r]]
                idle = is_idle(form, d)
                if idle and not shadow:
                    continue
                if form == "full":
                    vec = bool(d[0] & 0x8000)
                    T, Wa, Wb, D = (d[0] & 0x7fff) >> 3, d[1] >> 3, d[2] >> 3, d[3] >> 3
                    P00, P01, P11 = _inv(W[D: D + 4])
                    b0, b1 = W[Wb: Wb + 2], W[Wb + 2: Wb + 4]
                    for row in range(2 if shadow else (1 if vec else 2)):
                        a = W[Wa + 2 * row: Wa + 2 * row + 2]
                        g0, g1 = a[0] * P00 + a[1] * P01, a[0] * P01 + a[1] * P11
                        t = W[T + 2 * row: T + 2 * row + 2].copy()
                        t[0] -= g0 * b0[0] + g1 * b0[1]; t[1] -= g0 * b1[0] + g1 * b1[1]
                        if not idle and not (vec and row == 1):
                            stores.append((T + 2 * row, t))
                    continue
                d = [x >> 3 for x in d]
                if form == "half":
                    T, Wa, Wb, D = d
                    P00, P01, P11 = _inv(W[D: D + 4])
                    a = W[Wa: Wa + 2]; b0, b1 = W[Wb: Wb + 2], W[Wb + 2: Wb + 4]
                    g0, g1 = a[0] * P00 + a[1] * P01, a[0] * P01 + a[1] * P11
                    t = W[T: T + 2].copy()
                    t[0] -= g0 * b0[0] + g1 * b0[1]; t[1] -= g0 * b1[0] + g1 * b1[1]
                    out = [(T, t)]
                elif form == "quarter":
                    T, Wa, Wb, D = d
                    P00, P01, P11 = _inv(W[D: D + 4])
                    a = W[Wa: Wa + 2]; b0 = W[Wb: Wb + 2]
                    g0, g1 = a[0] * P00 + a[1] * P01, a[0] * P01 + a[1] * P11
                    out = [(T, np.array([W[T] - (g0 * b0[0] + g1 * b0[1])]))]
                elif form == "inv":
                    D, Y = d[0], d[1]
                    P00, P01, P11 = _inv(W[D: D + 4])
                    y = W[Y: Y + 2]
                    out = [(D, np.array([P00, P01, P01, P11])), (Y, np.array([P00 * y[0] + P01 * y[1], P01 * y[0] + P11 * y[1]]))]
                elif form == "bwd_half":
                    Yi, Wk, Pr, Ya = d
                    w0, w1 = W[Wk: Wk + 2], W[Wk + 2: Wk + 4]
                    pr = W[Pr: Pr + 2]; x = W[Ya: Ya + 2]
                    u0, u1 = w0[0] * x[0] + w1[0] * x[1], w0[1] * x[0] + w1[1] * x[1]
                    out = [(Yi, np.array([W[Yi] - (pr[0] * u0 + pr[1] * u1)]))]
                else:
                    Yi, Wk, P, Ya = d
                    w0, w1 = W[Wk: Wk + 2], W[Wk + 2: Wk + 4]
                    p0, p1 = W[P: P + 2], W[P + 2: P + 4]
                    x = W[Ya: Ya + 2]
                    u0, u1 = w0[0] * x[0] + w1[0] * x[1], w0[1] * x[0] + w1[1] * x[1]
                    y = W[Yi: Yi + 2].copy()
                    y[0] -= p0[0] * u0 + p0[1] * u1; y[1] -= p1[0] * u0 + p1[1] * u1
                    out = [(Yi, y)]
                if not idle:
                    stores += out
            for off, v in stores:
                W[off: off + len(v)] = v
    return W


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def check_case(case, variant=0, order=None, seed=1):
    s = si.symbolic(case, variant, order)
    im = task_image(case, variant, order)
    assert (im["rw"], im["nb"], im["nws"], im["off_rhs"], im["npass"], im["npass_upd"], im["npass_inv"], im["npass_updh"], im["npass_updq"], im["bwd_half"]) == \
           (s.rw, s.nb, s.nws, s.off_rhs, s.npass, s.npass_upd, s.npass_inv, s.npass_updh, s.npass_updq, s.bwd_half)
    assert im["scen_doubles"] >= s.nws + 2
    n_idle = 0
    for p in range(im["npass"]):
        form = form_of(im, p)
        lanes = [[int(x) for x in im["tasks"][p, r]] for r in range(im["rw"])]
        idle = [is_idle(form, d) for d in lanes]
        active = [d for d, i in zip(lanes, idle) if not i]
        assert active, (p, "a pass without a task")
        active_of_group = {g: [d for r, d in enumerate(lanes) if not idle[r] and READ_GROUP[r] == g] for g in range(4)}
        ro = READ_ONLY_FIELDS.get(form, (1, 2, 3))
        for r, d in enumerate(lanes):
            # in bounds and aligned, idle or not: the shadowing kernel reads through every lane's fields
            for f, add, nbytes, align in READS[form]:
                off = (d[0] & 0x7fff) if (form == "full" and f == 0) else d[f]
                assert off % align == 0, (p, r, f, off)
                # the full form's second rows of T and Wa are read for every lane: an rhs task reads 16 bytes behind its pair, still the scenario's LDS
                limit = 8 * (im["nws"] + 2) if (form == "full" and f in (0, 1)) else 8 * im["nws"]
                assert 0 <= off + add and off + add + nbytes <= limit, (p, r, f, off)
            # the non-idle lanes are exactly relmc_debug_symbolic's tasks (offsets in doubles there)
            sym = [int(x) for x in s.tasks[p, r]]
            if idle[r]:
                n_idle += 1
                assert sym[0] == 0xffff, (p, r)
                # an idle lane's read fields are those of an active lane of its pass and of its own read group (then every copied operand is a
                # broadcast inside the group, in every scenario row); only where no lane of the group has a task, of any active lane of the pass.
                # On the 16-lane tile the lanes of a pass are one 16-lane row of the wavefront per scenario, so "the same row" holds throughout.
                mates = active_of_group[READ_GROUP[r]] or active
                assert any(all(d[f] == a[f] for f in ro) for a in mates), (p, r, d)
                if form != "inv":
                    assert d[0] == d[3]
                if form == "inv":
                    assert d[2] == IDLE_INV and d[3] == IDLE_INV
            else:
                assert sym[0] != 0xffff, (p, r)
                back = [((d[0] & 0x7fff) >> 3) | (d[0] & 0x8000) if form == "full" else d[0] >> 3] + [d[k] >> 3 for k in (1, 2, 3)]
                assert back == sym, (p, r, back, sym)
                # no real task matches the idle marker
                if form == "inv":
                    assert d[2] == 0 and d[3] == 0
                else:
                    assert d[0] != d[3]
    assert n_idle == int((s.tasks[:, :, 0] == 0xffff).sum())
    # one Newton system, and one whose shadowed (and real) arithmetic overflows: a pivot block scaled to 1e-300
    rng = np.random.default_rng(seed)
    W0, A, rhs = si.random_system(s, rng)
    W1 = W0.copy(); W1[0:4] *= 1e-300                                   # bus 0 is eliminated first: its pivot block reaches the inverse as it is
    for W in (W0, W1):
        with np.errstate(all="ignore"):
            x_ref = si.solve(s, W)
        masked = run_image(im, W, shadow=False)
        shadow = run_image(im, W, shadow=True)
        assert np.array_equal(_bits(masked[s.off_rhs: s.off_rhs + 2 * s.nb]), _bits(x_ref))
        assert np.array_equal(_bits(shadow), _bits(masked))
    assert not np.isfinite(run_image(im, W1, shadow=True)).all()          # the overflow did happen
    b_tasks, b_shadow = _model_bounds(im)                                 # the placement model on the image (below)
    assert im["cost_masked"] <= im["cost_tasks"] <= im["cost_masked"] + b_tasks and im["cost_shadow"] <= im["cost_tasks"] + b_shadow
    return im


def test_rts24_image_rule_and_tuned_orders_and_retry_levels():
    case = case24.rts24()
    for variant, order in ((0, None), (0, case.elim_order), (1, None), (2, None)):
        im = check_case(case, variant, order, seed=10 + variant)
        assert im["tile"] == 0 and im["rw"] == 16


def test_rts96_image_on_the_wide_tile():
    case = case96.rts96()
    for variant, order in ((0, None), (0, case.elim_order)):
        im = check_case(case, variant, order, seed=20)
        assert im["tile"] == 1 and im["rw"] == 64


@pytest.mark.parametrize("seed,nb,chords,ng,loads", [(1, 2, 0, 2, 1), (8, 5, 2, 3, 3), (2, 7, 3, 4, 4), (9, 9, 3, 4, 4), (4, 30, 14, 12, 14)])
def test_small_random_networks_where_most_lanes_are_idle(seed, nb, chords, ng, loads):
    case = random_case(np.random.default_rng(100 + seed), nb, chords, ng, loads)
    im = check_case(case, 0, None, seed)
    assert im["rw"] == 16


def _model_bounds(im):
    """What the shadowing kernel may add to the modelled conflict cycles, by counting new addresses: a new distinct address in one read
    instruction raises the largest multiplicity of one bank slot of one read group by at most one, i.e. costs at most one cycle.
      * Tasks: a right-hand-side task of a full-form pass now reads its second rows (T + 16, Wa + 16): one new address per task, scenario row
        of the wavefront and each of the two reads.
      * Shadows: the idle lanes of one read group carry the same descriptor, so per scenario row they add ONE address to a read whose field
        they do not copy (the target field, which holds the marker: both rows in the full form, one read otherwise; none in an inversion),
        and one to every read of the pass if no lane of their group has a task (nothing to broadcast from); nothing otherwise."""
    rows = 64 // im["rw"]
    b_tasks = b_shadow = 0
    for p in range(im["npass"]):
        form = form_of(im, p)
        lanes = [[int(x) for x in im["tasks"][p, r]] for r in range(im["rw"])]
        idle = [is_idle(form, d) for d in lanes]
        if form == "full":
            b_tasks += 2 * rows * sum(1 for d, i in zip(lanes, idle) if not i and d[0] & 0x8000)
        n_reads = {"full": 8, "half": 6, "quarter": 5, "inv": 3, "bwd": 6, "bwd_half": 5}[form]
        n_marker = {"full": 2, "inv": 0}.get(form, 1)
        for g in set(READ_GROUP[: im["rw"]]):
            has_idle = any(idle[r] for r in range(im["rw"]) if READ_GROUP[r] == g)
            has_task = any(not idle[r] for r in range(im["rw"]) if READ_GROUP[r] == g)
            if has_idle:
                b_shadow += rows * (n_marker if has_task else n_reads)
    return b_tasks, b_shadow


# the parent commit's placement model (relmc_debug_symbolic's conflict_after) of the shipped orders: the search runs before the idle lanes are
# rewritten and must come out as it did
PARENT_CONFLICT_AFTER = {24: 96, 73: 287}


@pytest.mark.parametrize("make", [case24.rts24, case96.rts96])
def test_placement_model_of_the_shipped_images(make):
    """The placement search's own figure (conflict_after) is the parent's.  The same model on the finished device image, in modelled extra LDS
    cycles per Newton step -- idle lanes masked / the tasks with every second row read / idle lanes shadowing: RTS-24 114 / 162 / 172,
    RTS-96 455 / 465 / 469.  So the shadowing kernel's modelled conflicts DO rise: by 48 (10) for the right-hand-side tasks' second rows,
    which every lane reads now, and by 10 (4) for the shadows' target field, which holds the marker instead of a copied address.  Both
    rises are held to the bounds of _model_bounds; what the hardware counted is in profiles/pass_shadow/README.md."""
    case = make()
    s = si.symbolic(case, 0, case.elim_order)
    assert s.conflict_after == PARENT_CONFLICT_AFTER[case.nb]
    im = task_image(case, 0, case.elim_order)
    b_tasks, b_shadow = _model_bounds(im)
    print(case.nb, "buses: masked", im["cost_masked"], "tasks, every row", im["cost_tasks"], "shadowing", im["cost_shadow"], "bounds", b_tasks, b_shadow)
    assert im["cost_masked"] <= im["cost_tasks"] <= im["cost_masked"] + b_tasks
    assert im["cost_shadow"] <= im["cost_tasks"] + b_shadow
