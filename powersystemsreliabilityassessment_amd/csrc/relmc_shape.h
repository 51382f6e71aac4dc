// relmc_shape.h — the SHAPE of a case as relmc_eval_kernel sees it: the dimensions, pass counts, gather lengths and workspace offsets that
// the kernel otherwise learns at run time (from the case tables in LDS and from EvalArgs).  The kernel takes them through a shape class:
//   ShapeDynamic        every field is the run-time value: the interpreter of any case that fits the tile
//   ShapeStaticT<V>     every field is a compile-time constant of V: loop bounds, guards and LDS sub-array offsets fold away.
//                       relmc_case_load selects such an instantiation only when EVERY field equals the loaded case's (shape_matches).
// The arithmetic, its order, the lane map, the LDS layout, the descriptors and the schedule do not depend on the shape class.
#pragma once
#include <stdint.h>

#include "relmc_dev.h"

namespace relmc {

// the fields, in the order of shape_of() / ShapeStaticT::values() / relmc_debug_shape (tests/test_shape_paths.py names them the same way)
enum ShapeField {
    SF_RW = 0, SF_NB, SF_NG, SF_NL, SF_NINJ, SF_NZERO, SF_OFF_RHS, SF_NPASS_UPD, SF_NPASS_UPDH, SF_NPASS_UPDQ, SF_NPASS_INV, SF_NPASS,
    SF_MAXDEG0, SF_MAXDEG1, SF_MAXINJ0, SF_MAXINJ1, SF_BWD_ALL_HALF, SF_STASH_OFF, SF_SCEN_DOUBLES, SF_COUNT,
    // behind what relmc_debug_shape exports: the fill blocks left to the clearing loop and those the bus-slot lanes clear (relmc_dev.h: nzero_res,
    // nfill_bus), and the lanes of the line slots and of either bus slot that store no block (nidle_line, nidle_bus_s; relmc_debug_fill_lanes
    // shows them all).  shape_matches compares them like every other field.
    SF_NZERO_RES = SF_COUNT, SF_NFILL_BUS, SF_NIDLE_LINE, SF_NIDLE_BUS0, SF_NIDLE_BUS1, SF_COUNT_ALL
};

// The kernel reads a field as SHAPE(field, run-time expression): a conditional on a constant of the shape class, of which the compiler emits
// the live arm only.  With ShapeDynamic the kernel is therefore the very program it was before the shape class existed; with a static shape
// the run-time expression of a fixed field is never evaluated.  A static shape fixes the field GROUPS of its mask and leaves the others at
// their run-time values (relmc_case_load compares every field all the same):
//   SG_PASS   the pass counts of the solver schedule          SG_GATHER  the gather lengths per bus slot
//   SG_DIM    nb, ng, nl, ninj, nzero, nzero_res, nfill_bus, nidle_* (guards, zero fill)     SG_OFF     off_rhs, stash_off, scen_doubles (LDS sub-array bases)
enum ShapeGroup { SG_PASS = 1, SG_GATHER = 2, SG_DIM = 4, SG_OFF = 8, SG_ALL = 15 };
#define SHAPE(field, dyn) ((SH::kMask & SH::grp_##field) != 0 ? (decltype(+(dyn)))SH::field : (dyn))
struct ShapeGroups {
    static constexpr int grp_npass_upd = SG_PASS, grp_npass_updh = SG_PASS, grp_npass_updq = SG_PASS, grp_npass_inv = SG_PASS, grp_npass = SG_PASS, grp_bwd_all_half = SG_PASS,
                         grp_maxdeg0 = SG_GATHER, grp_maxdeg1 = SG_GATHER, grp_maxinj0 = SG_GATHER, grp_maxinj1 = SG_GATHER,
                         grp_nb = SG_DIM, grp_ng = SG_DIM, grp_nl = SG_DIM, grp_ninj = SG_DIM, grp_nzero = SG_DIM, grp_nzero_res = SG_DIM, grp_nfill_bus = SG_DIM, grp_nidle_line = SG_DIM, grp_nidle_bus0 = SG_DIM, grp_nidle_bus1 = SG_DIM,
                         grp_off_rhs = SG_OFF, grp_stash_off = SG_OFF, grp_scen_doubles = SG_OFF;
};
struct ShapeDynamic : ShapeGroups {
    static constexpr int kMask = 0;
    // placeholders that no code reads
    static constexpr int nb = 0, ng = 0, nl = 0, ninj = 0, nzero = 0, nzero_res = 0, nfill_bus = 0, nidle_line = 0, nidle_bus0 = 0, nidle_bus1 = 0, off_rhs = 0, npass_upd = 0, npass_updh = 0, npass_updq = 0, npass_inv = 0, npass = 0,
                         maxdeg0 = 0, maxdeg1 = 0, maxinj0 = 0, maxinj1 = 0, bwd_all_half = 0, stash_off = 0, scen_doubles = 0;
};

// V: a struct of `static constexpr int` members named like the fields (relmc_shape_rts24.h); MASK: the groups compiled in
template <class V, int MASK = SG_ALL>
struct ShapeStaticT : ShapeGroups {
    static constexpr int kMask = MASK;
    static constexpr int nb = V::nb, ng = V::ng, nl = V::nl, ninj = V::ninj, nzero = V::nzero, nzero_res = V::nzero_res, nfill_bus = V::nfill_bus, nidle_line = V::nidle_line, nidle_bus0 = V::nidle_bus0, nidle_bus1 = V::nidle_bus1, off_rhs = V::off_rhs, npass_upd = V::npass_upd, npass_updh = V::npass_updh,
                         npass_updq = V::npass_updq, npass_inv = V::npass_inv, npass = V::npass, maxdeg0 = V::maxdeg0, maxdeg1 = V::maxdeg1, maxinj0 = V::maxinj0,
                         maxinj1 = V::maxinj1, bwd_all_half = V::bwd_all_half, stash_off = V::stash_off, scen_doubles = V::scen_doubles;
    static void values(int32_t* out)
    {
        out[SF_RW] = V::rw; out[SF_NB] = V::nb; out[SF_NG] = V::ng; out[SF_NL] = V::nl; out[SF_NINJ] = V::ninj; out[SF_NZERO] = V::nzero;
        out[SF_OFF_RHS] = V::off_rhs; out[SF_NPASS_UPD] = V::npass_upd; out[SF_NPASS_UPDH] = V::npass_updh; out[SF_NPASS_UPDQ] = V::npass_updq;
        out[SF_NPASS_INV] = V::npass_inv; out[SF_NPASS] = V::npass; out[SF_MAXDEG0] = V::maxdeg0; out[SF_MAXDEG1] = V::maxdeg1;
        out[SF_MAXINJ0] = V::maxinj0; out[SF_MAXINJ1] = V::maxinj1; out[SF_BWD_ALL_HALF] = V::bwd_all_half; out[SF_STASH_OFF] = V::stash_off;
        out[SF_SCEN_DOUBLES] = V::scen_doubles; out[SF_NZERO_RES] = V::nzero_res; out[SF_NFILL_BUS] = V::nfill_bus;
        out[SF_NIDLE_LINE] = V::nidle_line; out[SF_NIDLE_BUS0] = V::nidle_bus0; out[SF_NIDLE_BUS1] = V::nidle_bus1;
    }
};

// the same fields of a case image and its launch geometry, as relmc_case_load computed them (host)
template <class DC>
inline void shape_of(const DC& C, uint32_t stash_off, uint32_t scen_doubles, int32_t* out)
{
    out[SF_RW] = DC::ROWL; out[SF_NB] = C.nb; out[SF_NG] = C.ng; out[SF_NL] = C.nl; out[SF_NINJ] = C.ninj; out[SF_NZERO] = C.nzero;
    out[SF_OFF_RHS] = C.off_rhs; out[SF_NPASS_UPD] = C.npass_upd; out[SF_NPASS_UPDH] = C.npass_updh; out[SF_NPASS_UPDQ] = C.npass_updq;
    out[SF_NPASS_INV] = C.npass_inv; out[SF_NPASS] = C.npass; out[SF_MAXDEG0] = C.maxdeg_s[0]; out[SF_MAXDEG1] = C.maxdeg_s[1];
    out[SF_MAXINJ0] = C.maxinj_s[0]; out[SF_MAXINJ1] = C.maxinj_s[1]; out[SF_BWD_ALL_HALF] = C.bwd_half != 0 ? 1 : 0; out[SF_STASH_OFF] = (int32_t)stash_off;
    out[SF_SCEN_DOUBLES] = (int32_t)scen_doubles; out[SF_NZERO_RES] = C.nzero_res; out[SF_NFILL_BUS] = C.nfill_bus;
    out[SF_NIDLE_LINE] = C.nidle_line; out[SF_NIDLE_BUS0] = C.nidle_bus_s[0]; out[SF_NIDLE_BUS1] = C.nidle_bus_s[1];
}

template <class SH, class DC>
inline bool shape_matches(const DC& C, uint32_t stash_off, uint32_t scen_doubles)
{
    int32_t a[SF_COUNT_ALL], b[SF_COUNT_ALL];
    SH::values(a); shape_of(C, stash_off, scen_doubles, b);
    for (int k = 0; k < SF_COUNT_ALL; ++k) if (a[k] != b[k]) return false;
    return true;
}

}  // namespace relmc
