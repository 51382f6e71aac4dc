"""Which lane clears which fill-only block of the factor (csrc/relmc_dev.h: l_blk_fill, b_lane_fill; csrc/relmc_schedule.hip: fill_lanes), checked on
the CPU through `relmc_debug_fill_lanes`: the shipped RTS-24 image, RTS-96, the random networks of tests/test_schedule.py and networks whose
spare lanes do not suffice, so that some blocks stay with the clearing loop."""
import ctypes as C

import numpy as np
import pytest

from powersystemsreliabilityassessment_amd import _abi, _lib, case24, case96
from tests import schedule_interp as si
from tests.test_random_cases import random_case

LF_OWNER = 2


def fill_lanes(case, variant=0):
    f = _lib.load().relmc_debug_fill_lanes
    f.restype = C.c_int32
    f.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    holder = _abi.CaseHolder(case)
    order = getattr(case, "elim_order", None) if variant == 0 else None
    o = None if order is None else np.ascontiguousarray(order, dtype=np.int32)
    hdr = np.full(24, -1, np.int32)
    lbf, blf, bl = np.zeros(256, np.uint16), np.zeros(256, np.uint16), np.zeros(256, np.uint8)
    rc = f(C.byref(holder.desc), variant, None if o is None else o.ctypes.data, 0 if o is None else int(o.size), hdr.ctypes.data, lbf.ctypes.data,
           blf.ctypes.data, bl.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"relmc_debug_fill_lanes failed ({rc})")
    h = dict(zip(["rw", "nb", "nl", "nzero", "nzero_res", "nfill_line", "nfill_bus", "nlt", "nbt", "static_nzero_res", "static_nfill_bus",
                  "nidle_line", "nidle_bus0", "nidle_bus1", "static_nidle_line", "static_nidle_bus0", "static_nidle_bus1"], map(int, hdr)))
    return h, lbf[: h["nlt"]].astype(int), blf[: h["nbt"]].astype(int), bl[: h["nbt"]].astype(int)


def check(case, variant=0):
    """The three properties of the assignment; returns the header."""
    s = si.symbolic(case, variant, order=getattr(case, "elim_order", None) if variant == 0 else None)
    h, lbf, blf, bl = fill_lanes(case, variant)
    nb, nl, nres, nline, nbus = h["nb"], h["nl"], h["nzero_res"], h["nfill_line"], h["nfill_bus"]
    assert (nb, nl, h["nzero"]) == (s.nb, s.nl, s.nzero) and nres + nline + nbus == s.nzero
    zero = [int(z) for z in s.zero_off]
    owner = np.zeros(h["nlt"], bool); owner[:nl] = ((s.l_info >> 24) & LF_OWNER) != 0
    l_blk = np.full(h["nlt"], 0xffff); l_blk[:nl] = s.l_blk                      # 0xffff off an owner (relmc_debug_symbolic)
    # what the kernels without the assignment read stays: an owner's lane keeps its block, a bus' lane its bus
    assert np.array_equal(lbf[owner], l_blk[owner]) and np.array_equal(blf[bl != 0xff], bl[bl != 0xff])
    assert sorted(bl[bl != 0xff]) == list(range(nb))
    # no assigned lane holds an owner line or a bus
    line_fill = [int(v) for v in lbf[~owner] if v != 0xffff]
    bus_fill = [4 * int(v) for v in blf[bl == 0xff] if v != 0xffff]
    assert all(v >= nb for v in blf[bl == 0xff]), "a bus-slot lane tells a fill block from a bus by position >= nb"
    # every fill block is cleared exactly once: by a spare lane, or by the loop over the first nzero_res entries of zero_off
    assert len(line_fill) == nline and len(bus_fill) == nbus
    assert sorted(line_fill + bus_fill + zero[:nres]) == sorted(zero) and len(set(zero)) == len(zero)
    # spare lanes are used up before a block is left to the loop
    spare_line, spare_bus = int((~owner).sum()), int((bl == 0xff).sum())
    assert nline <= spare_line and nbus <= spare_bus and nline + nbus == min(s.nzero, spare_line + spare_bus)
    # the lanes that store no block at all, per site (a slot without one needs no predicate on its block stores)
    rw = h["rw"]
    assert h["nidle_line"] == int((lbf == 0xffff).sum()) and [h["nidle_bus0"], h["nidle_bus1"]] == [int((blf[rw * t:rw * t + rw] == 0xffff).sum()) for t in (0, 1)]
    # diagonal, owner and fill blocks together cover every block of the workspace once
    blocks = [int(v) for v in blf if v != 0xffff] + [int(v) // 4 for v in lbf if v != 0xffff] + [z // 4 for z in zero[:nres]]
    assert all(int(v) % 4 == 0 for v in lbf if v != 0xffff)
    assert sorted(blocks) == list(range(nb + s.noff)), (len(blocks), nb + s.noff)
    return h


def test_rts24_every_fill_block_has_a_spare_lane_and_the_header_says_so():
    h = check(case24.rts24())
    assert (h["rw"], h["nzero"], h["nzero_res"]) == (16, 20, 0)
    for k in ("nzero_res", "nfill_bus", "nidle_line", "nidle_bus0", "nidle_bus1"):                  # relmc_shape_rts24.h
        assert h[k] == h["static_" + k], (k, h[k], h["static_" + k])
    for variant in (1, 2):
        check(case24.rts24(), variant)


def test_rts96():
    for variant in (0, 1, 2):
        check(case96.rts96(), variant)


@pytest.mark.parametrize("seed,nb,chords,ng,loads", [(1, 2, 0, 2, 1), (2, 7, 3, 4, 4), (3, 19, 8, 9, 10), (4, 30, 14, 12, 14), (5, 60, 25, 30, 35),
                                                     (6, 100, 26, 40, 50), (7, 120, 6, 40, 60)])
def test_random_networks(seed, nb, chords, ng, loads):
    case = random_case(np.random.default_rng(100 + seed), nb, chords, ng, loads)
    for variant in (0, 1, 2):
        try:
            check(case, variant)
        except RuntimeError as e:                       # a further order may not fit the tile (tests/test_schedule.py)
            assert variant != 0 and "relmc_debug_symbolic failed (-4)" in str(e), e


@pytest.mark.parametrize("seed,nb,chords", [(11, 32, 16), (12, 31, 17), (13, 120, 7)])
def test_networks_whose_spare_lanes_do_not_suffice(seed, nb, chords):
    """Tiles filled (almost) to the last bus and line slot: few spare lanes, so fill blocks are left to the loop."""
    case = random_case(np.random.default_rng(seed), nb, chords, 8, 8)
    h = check(case)
    assert h["nzero_res"] > 0, h
