// relmc_area_variable_devfn.h — what the weather-year instantiations of relmc_hl1_area_kernel (relmc_area_kernels.h, which includes this
// header ahead of its kernel) have of their own: weather-year resources and storages in the areas of the HL1 multi-area chronology
// (relmc_hl1_area_var, contract in include/relmc.h).  The by-value argument struct, the rows of the dynamic LDS, relmc_hl1_seq_storage's
// step rule applied area by area AFTER the transfers, and the year close of both record rows.  An extension beyond the reference, whose
// areas hold dispatchable units only.  No kernel is defined here; the weather pick and the storage leaves are relmc_hl1_storage_devfn.h's.
#pragma once
#include "relmc_hl1_chrono.h"
#include "relmc_hl1_storage_devfn.h"

namespace relmc {

// The storages with their areas, the load levels, the resource scales with their areas and the weather library, passed BY VALUE as a
// kernel argument (as Hl1VarArgs): every read of them is a scalar load from the kernel argument segment.  Entries at or above the counts
// are zero and never read.
struct AreaVarArgs {
    relmc_hl1_storage st[RELMC_HL1_MAX_STORAGE];
    int32_t sarea[RELMC_HL1_MAX_STORAGE];                   // 0-based area of storage i
    double rscale[RELMC_HL1_VAR_MAX_RESOURCES];
    int32_t rarea[RELMC_HL1_VAR_MAX_RESOURCES];             // 0-based area of resource r
    double lscale[AREA_MAX], lshift[AREA_MAX];
    const double* out;                   // [n_weather][n_res][H], fewer than 2^31 values (relmc_hl1_area_var_load): indexed in 32 bits
    const double* wload;                 // [n_weather][n_areas][H] (fewer than 2^31 values), or nullptr: the curves of relmc_hl1_area_load
    int32_t n_storage, n_res, n_weather, pick;
};

// Rows of 64 doubles of the kernel's dynamic LDS ahead of the window masks, shared by the host's launch and the kernel's pointers:
//   aE [na + 1]   EUE partials of the open year, per record row
//   aD, aC [na + 1] each, xy [na]   (n_storage > 0 only) discharged / charged MWh partials, and the step's x or y sum of each area
//   mg [na]       the step's margins
//   R  [na * na]  (INTERCONNECTED only) residual capacities of the transfer solve
__host__ __device__ inline int area_var_lds_rows(int na, bool inter, bool stor)
{
    return (na + 1) + (stor ? 2 * (na + 1) + na : 0) + na + (inter ? na * na : 0);
}

// a value every lane holds alike (an LDS read at a wave-uniform address), moved to scalar registers: the tests on it are scalar branches
DEVFI double area_var_uniform(double v)
{
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
}

// the areas (bit a) that hold a storage able to discharge (low half) / not settled (high half, << 16)
DEVFI uint32_t area_var_can(const AreaVarArgs& A, int ns, uint32_t bits)
{
    uint32_t can = 0u;
    hl1_storage_each([&](auto ic) {
        constexpr int i = decltype(ic)::value;
        if (i < ns) can |= (((bits >> i) & 1u) | (((bits >> (8 + i)) & 1u) << 16)) << A.sarea[i];
    });
    return can;
}

// Step j of the group, visited by the whole wave: every storage in array order acts on the margin left in ITS area, mgw[area * 64 + j]
// (< 0: the need -m, the contract's short step; > 0: the surplus, its long step), which it reads and writes back; the step's x or y is
// added to xyw[area * 64 + j].  soc holds storage i's state of charge in lane i; z is a zero the compiler cannot see through, so that a
// storage's data is read where it is used.  Areas do not interact here (the transfers are done), so the array order over all storages is
// each area's own order.
DEVFI void area_var_storage_step(const AreaVarArgs& A, int ns, int z, int lane, int j, double* __restrict__ mgw, double* __restrict__ xyw,
                                 double& soc, uint32_t& bits)
{
    hl1_storage_each([&](auto ic) {
#pragma clang fp contract(off)
        constexpr int i = decltype(ic)::value;
        if (i < ns && ((bits >> i) & 0x101u)) {              // wave-uniform
            const relmc_hl1_storage& p = A.st[i + z];
            const int at = (A.sarea[i + z] & (AREA_MAX - 1)) * 64 + j;
            const double m = area_var_uniform(mgw[at]);
            if (m < 0.0 && ((bits >> i) & 1u)) {
                const double need = -m, eta = p.eta_discharge, s = hl1_storage_readlane(soc, i);
                const double avail = __builtin_fmin(p.discharge_mw, s * eta);
                const double x = __builtin_fmin(avail, need);
                const double t = __builtin_fmax(0.0, s - x / eta);
                const double left = need - x;
                const double xs = area_var_uniform(xyw[at]) + x;
                if (lane == j) { mgw[at] = -left; xyw[at] = xs; }
                soc = lane == i ? t : soc;
                bits = (bits & ~(0x101u << i)) | hl1_storage_bits(p, t, i);
            } else if (m > 0.0 && ((bits >> (8 + i)) & 1u)) {
                const double eta = p.eta_charge, cap = p.energy_mwh, s = hl1_storage_readlane(soc, i);
                const double room = (cap - s) / eta;
                const double y = __builtin_fmin(__builtin_fmin(p.charge_mw, room), m);
                const double t = __builtin_fmin(cap, s + y * eta);
                const double left = m - y;
                const double ys = area_var_uniform(xyw[at]) + y;
                if (lane == j) { mgw[at] = left; xyw[at] = ys; }
                soc = lane == i ? t : soc;
                bits = (bits & ~(0x101u << i)) | hl1_storage_bits(p, t, i);
            }
        }
    });
}

// Row r of the wave's open year: the fixed-order butterflies of the lane partials (area_close_year's, over both records); lane 0 stores
// (loss hours, EUE, loss events) to out0 and (served hours, MWh discharged, MWh charged) to out1; the row restarts at zero.  Without
// storages the row has no partials of the second record (dD: nullptr) and its sums are 0.0.
DEVFI void area_var_close_year(double& e_lds, double* __restrict__ dD, double* __restrict__ dC, int& l, int& f, int& sv,
                               double* __restrict__ out0, double* __restrict__ out1)
{
    double e = e_lds, d = dD ? *dD : 0.0, c = dD ? *dC : 0.0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { e += __shfl_xor(e, off); d += __shfl_xor(d, off); c += __shfl_xor(c, off); }
    if (threadIdx.x == 0) {
        out0[0] = (double)l; out0[1] = e; out0[2] = (double)f;
        out1[0] = (double)sv; out1[1] = d; out1[2] = c;
    }
    e_lds = 0.0; l = f = sv = 0;
    if (dD) { *dD = 0.0; *dC = 0.0; }
}

// What the kernel's setup reads of the argument: its by-value parameter is a pack, empty in the instantiations without weather years, so
// each of these has a form without an argument that gives nothing (no storages, no resources, no library)
DEVFI int area_var_ns() { return 0; }
DEVFI int area_var_nres() { return 0; }
DEVFI const double* area_var_wload() { return nullptr; }
DEVFI const double* area_var_out() { return nullptr; }
DEVFI int area_var_ns(const AreaVarArgs& V) { return V.n_storage < RELMC_HL1_MAX_STORAGE ? V.n_storage : RELMC_HL1_MAX_STORAGE; }
DEVFI int area_var_nres(const AreaVarArgs& V) { return V.n_res < RELMC_HL1_VAR_MAX_RESOURCES ? V.n_res : RELMC_HL1_VAR_MAX_RESOURCES; }
DEVFI const double* area_var_wload(const AreaVarArgs& V) { return V.wload; }
DEVFI const double* area_var_out(const AreaVarArgs& V) { return V.out; }
DEVFI const AreaVarArgs& area_var_args(const AreaVarArgs& V) { return V; }
}  // namespace relmc
