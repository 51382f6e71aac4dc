// relmc_shape_rts24.h — the shape of the shipped IEEE RTS-24 case (case24.rts24() under its tuned elimination order) on the 16-lane tile,
// as relmc_case_load computes it.  Written by `python scripts/shape_header.py`; tests/test_shape_paths.py fails when these numbers and
// relmc_debug_shape of case24.rts24() disagree.  A case that differs in any field runs through ShapeDynamic.
#pragma once
#include "relmc_shape.h"

namespace relmc {

struct ShapeRts24Values {
    static constexpr int rw = 16;
    static constexpr int nb = 24;
    static constexpr int ng = 33;
    static constexpr int nl = 38;
    static constexpr int ninj = 50;
    static constexpr int nzero = 20;
    static constexpr int off_rhs = 312;
    static constexpr int npass_upd = 12;
    static constexpr int npass_updh = 3;
    static constexpr int npass_updq = 1;
    static constexpr int npass_inv = 2;
    static constexpr int npass = 21;
    static constexpr int maxdeg0 = 5;
    static constexpr int maxdeg1 = 3;
    static constexpr int maxinj0 = 7;
    static constexpr int maxinj1 = 1;
    static constexpr int bwd_all_half = 0;
    static constexpr int stash_off = 360;
    static constexpr int scen_doubles = 526;
    static constexpr int nzero_res = 0;
    static constexpr int nfill_bus = 6;
    static constexpr int nidle_line = 0;
    static constexpr int nidle_bus0 = 0;
    static constexpr int nidle_bus1 = 2;
};
#ifndef RELMC_SHAPE_MASK
// The field groups compiled into the specialised kernel (ablation builds: -DRELMC_SHAPE_MASK=<ShapeGroup bits>).  The gather lengths stay
// run-time values: without the early exits of the gather loops the compiler issues a bus' record loads as one batch and scratch grows from
// 176 to 440 bytes per lane (DESIGN_HISTORY.md).
#define RELMC_SHAPE_MASK (SG_PASS | SG_DIM | SG_OFF)
#endif
using ShapeRts24 = ShapeStaticT<ShapeRts24Values, RELMC_SHAPE_MASK>;

}  // namespace relmc
