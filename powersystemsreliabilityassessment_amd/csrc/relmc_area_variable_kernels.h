// relmc_area_variable_kernels.h — weather-year resources and storages in the areas of the HL1 multi-area chronology (relmc_hl1_area_var,
// contract in include/relmc.h): relmc_hl1_area_kernel's chronology and transfer solve, relmc_hl1_var_kernel's weather years and resource
// outputs in each area's capacity, and relmc_hl1_seq_storage's step rule applied area by area AFTER the transfers.  An extension beyond
// the reference, whose areas hold dispatchable units only.
// The transfer solve (area_bfs, area_solve, area_tie_residual) is relmc_area_kernels.h's, whose kernel is a template and is not
// instantiated here; the weather pick and the storage leaves are relmc_hl1_storage_devfn.h's.  The area-wise storage step is this unit's.
#pragma once
#include "relmc_area_kernels.h"
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

// Chain c = first_chain + blockIdx.x: one wavefront per workgroup, one chain per wavefront.  The cursor slots and the window fill are a
// COPY of relmc_hl1_area_kernel's (relmc_area_kernels.h, which says what they do), on purpose: sharing them between kernels cost the
// sequential kernel 1.6-3 % twice.  Per 64-step group:
//   parallel stage, one step per lane
//     weather    the lane keeps (yw, w * H) of its chain year and works the pick out only when the year changes (relmc_hl1_var_kernel)
//     loads      L_a = lscale[a] * base_a(w, h) + lshift[a] of every area into the margin slots, and the first two resource outputs, are
//                read AHEAD of the capacity sum, whose work hides their latency; 32-bit library indices
//     capacity   the units walk with the area close-outs; a close-out adds the area's resources r ascending and leaves m_a = cap_a - L_a
//     transfers  the solve only on lanes with a negative margin under INTERCONNECTED: the contract puts the ties before the storages, so
//                the solve needs no state of charge and stays in this stage
//   quiet test   no lane has a margin < 0 left and every storage is settled: the group is skipped on a wave-uniform branch; years are
//                closed lazily, their sums bitwise what they would be (+ 0.0)
//   serial stage in step order, only the steps on which a storage can act (an area short that holds a storage able to discharge, or long
//                with one not settled): area_var_storage_step.  States of charge in the lanes of one register pair.
//   then the flags, rising edges, wave-uniform counts and year closes of relmc_hl1_area_kernel, for both record rows.
// Dynamic LDS: area_var_lds_rows rows of 64 doubles, then the masks [nw (+ 1 with TIES)][HL1_SEQ_WINDOW].
// Records: rec[slice][chain of the launch * years + year][3], slices `stride` records apart: slice r = row r's (lole, eue, lolf),
// slice n_areas + 1 + r = row r's (served_hours, discharged_mwh, charged_mwh); row n_areas is the system.
template <bool TIES>
__global__ void __launch_bounds__(64) relmc_hl1_area_var_kernel(const AreaCase* __restrict__ A, const AreaTies* __restrict__ TL,
                                                                const double* __restrict__ load, uint64_t seed, uint64_t first_chain,
                                                                int32_t years, int32_t start, int32_t policy, int32_t flow, int64_t stride,
                                                                const AreaVarArgs V, double* __restrict__ rec)
{
    constexpr int NS = TIES ? 3 : 2;                         // cursor slots per lane: units lane, lane + 64, and tie `lane`
    constexpr int W = HL1_SEQ_WINDOW;
    extern __shared__ double lds[];
    const int lane = threadIdx.x;
    const int64_t cl = blockIdx.x;
    const uint64_t chain = first_chain + (uint64_t)cl;
    const int ngen = A->ngen, H = A->nhours, na = A->n_areas, nw = (ngen + 31) >> 5, nslot = ngen > 64 ? 2 : 1;
    const bool inter = policy == RELMC_HL1_AREA_INTERCONNECTED;
    const int ns = V.n_storage < RELMC_HL1_MAX_STORAGE ? V.n_storage : RELMC_HL1_MAX_STORAGE;
    const int nres = V.n_res < RELMC_HL1_VAR_MAX_RESOURCES ? V.n_res : RELMC_HL1_VAR_MAX_RESOURCES;
    const bool stor = ns > 0;
    const int rows0 = na + 1, rowsS = stor ? 2 * (na + 1) + na : 0;
    double* const aE = lds + lane;                           // aE[r * 64]: this lane's EUE partial of row r in the open year ycur
    double* const aD = lds + 64 * rows0 + lane;              // stor only: MWh discharged / charged partials of row r, and
    double* const aC = aD + 64 * (na + 1);
    double* const xyw = lds + 64 * (rows0 + 2 * (na + 1));   //   xyw[a * 64 + j]: the x or y sum of area a in step j of the group
    double* const mgw = lds + 64 * (rows0 + rowsS);          // mgw[a * 64 + j]: the margin of area a in step j
    double* const mg = mgw + lane;
    double* const R = mgw + 64 * na + lane;
    uint32_t (*const seg)[W] = reinterpret_cast<uint32_t (*)[W]>(lds + 64 * area_var_lds_rows(na, inter, stor));
    const double* __restrict__ const lcurve = V.wload ? V.wload : load;      // base_a(w, h) = lcurve[(w * na * H & lmask) + a * H + h]
    const uint32_t lmask = V.wload ? ~0u : 0u;
    const double* __restrict__ const rout = V.out;
    const int64_t nsteps = (int64_t)years * H;
    double* const out = rec + (size_t)cl * (size_t)years * 3;

    bool down[NS], mine[NS];
    double tn[NS], mf[NS], mr[NS];
    int ev[NS];
    int64_t since[NS];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int k = lane + 64 * s;
        mine[s] = k < ngen;
        mf[s] = mine[s] ? A->mttf[k] : 1.0; mr[s] = mine[s] ? A->mttr[k] : 1.0;
        down[s] = false; ev[s] = 0; since[s] = 1; tn[s] = 0.0;
        if (mine[s]) {
            if (start == RELMC_HL1_START_STATIONARY) { down[s] = hl1_seq_u(chain, k, 0, seed) < A->q[k]; ev[s] = 1; }
            tn[s] = __dmul_rn(-(down[s] ? mr[s] : mf[s]), log(hl1_seq_u(chain, k, ev[s], seed)));    // T_1 (= 0 + duration)
            ++ev[s];
        }
    }
    if constexpr (TIES) {                                    // slot 2: tie `lane`, component AREA_TIE_DRAW_BASE + lane = lane + 64 * 2
        const int k = AREA_TIE_DRAW_BASE + lane;
        mine[2] = lane < TL->n_ties && TL->mttf[lane & (AREA_TIE_MAX - 1)] < __builtin_inf();
        mf[2] = mine[2] ? TL->mttf[lane] : 1.0; mr[2] = mine[2] ? TL->mttr[lane] : 1.0;
        down[2] = false; ev[2] = 0; since[2] = 1; tn[2] = 0.0;
        if (mine[2]) {
            if (start == RELMC_HL1_START_STATIONARY) { down[2] = hl1_seq_u(chain, k, 0, seed) < TL->q[lane]; ev[2] = 1; }
            tn[2] = __dmul_rn(-(down[2] ? mr[2] : mf[2]), log(hl1_seq_u(chain, k, ev[2], seed)));
            ++ev[2];
        }
    }

    double soc = 0.0;                                        // storage i's state of charge (MWh) in lane i
    uint32_t bits = 0u;                                      // hl1_storage_bits of every storage (wave-uniform)
    hl1_storage_each([&](auto ic) {
        constexpr int i = decltype(ic)::value;
        if (i < ns) { soc = lane == i ? V.st[i].soc0_mwh : soc; bits |= hl1_storage_bits(V.st[i], V.st[i].soc0_mwh, i); }
    });
    int cL[AREA_MAX + 1], cF[AREA_MAX + 1], cS[AREA_MAX + 1];   // the wave's loss hours / events / served hours of the open year, per row (uniform)
#pragma unroll
    for (int r = 0; r <= AREA_MAX; ++r) cL[r] = cF[r] = cS[r] = 0;
    for (int r = 0; r <= na; ++r) {
        aE[r * 64] = 0.0;
        if (stor) { aD[r * 64] = 0.0; aC[r * 64] = 0.0; }
    }
    int ycur = 0, gy = 0, gh = 0;
    int yw = -1;                                             // this lane's cached chain year, and
    uint32_t wb = 0u;                                        // w * H of its weather year w
    uint32_t prev = 0u;                                      // loss mask of the step before the group (none before step 1)
    const auto close = [&](int r) {
        area_var_close_year(aE[r * 64], stor ? aD + r * 64 : nullptr, stor ? aC + r * 64 : nullptr, cL[r], cF[r], cS[r],
                            out + (size_t)r * (size_t)stride * 3 + (size_t)ycur * 3,
                            out + (size_t)(na + 1 + r) * (size_t)stride * 3 + (size_t)ycur * 3);
    };
    for (int64_t w0 = 1; w0 <= nsteps; w0 += W) {
        const int64_t w1 = w0 + W;
        const int wlen = nsteps - w0 + 1 < W ? (int)(nsteps - w0 + 1) : W;
        for (int q = 0; q < nw + (TIES ? 1 : 0); ++q)
            for (int i = lane; i < W; i += 64) seg[q][i] = 0u;
        hl1_seq_wave_sync();
        // (1) down intervals [ceil(T_odd), ceil(T_even)) of the window
#pragma unroll
        for (int s = 0; s < NS; ++s) {                       // unrolled: the cursors stay in registers
            if (s < 2 && s >= nslot) { if constexpr (TIES) continue; else break; }
            bool more = mine[s];
            while (__any(more)) {
                int fb = 0, fe = 0;
                if (more) {
                    // the transition takes effect from step c on; a tie may be given an MTTF far beyond any run (1e30 h): such a T
                    // has no int64 image and means "never"
                    const int64_t c = TIES && s == 2 && !(tn[s] < 9.0e18) ? INT64_MAX : (int64_t)__builtin_ceil(tn[s]);
                    if (down[s]) {
                        const int64_t a = since[s] > w0 ? since[s] : w0, b = c < w1 ? c : w1;
                        if (b > a) { fb = (int)(a - w0); fe = (int)(b - w0); }
                    }
                    if (c >= w1) more = false;                                    // the cursor waits for a later window
                    else {
                        down[s] = !down[s]; since[s] = c;
                        const double l = log(hl1_seq_u(chain, lane + 64 * s, ev[s], seed));
                        tn[s] = __dadd_rn(tn[s], __dmul_rn(-(down[s] ? mr[s] : mf[s]), l));   // no FMA: the host model rounds the same way
                        ++ev[s];
                    }
                }
                for (uint64_t pend = __ballot(fe > fb); pend; pend &= pend - 1) {
                    const int src = __builtin_ctzll(pend);
                    const int sb = __builtin_amdgcn_readlane(fb, src), se = __builtin_amdgcn_readlane(fe, src), sk = src + 64 * s;
                    uint32_t* const row = seg[TIES && s == 2 ? nw : sk >> 5];
                    const uint32_t bit = 1u << (sk & 31);
                    for (int h = sb + lane; h < se; h += 64) row[h] |= bit;       // se <= W: inside the window's row
                }
            }
        }
        hl1_seq_wave_sync();
        // (2) one step per lane
        for (int g = 0; g < wlen; g += 64) {
            const int i = g + lane;                          // < W: g is a multiple of 64 below wlen <= W
            const bool valid = i < wlen;
            int h = gh + lane, y = gy;
            while (h >= H) { h -= H; ++y; }
            uint32_t sw = 0u, lw = 0u;                       // bit a: area a is short (m'_a < 0) / long (m'_a > 0) after the transfers
            if (valid) {                                     // y < years, h < H: every read below is inside its table
                if (y != yw) { yw = y; wb = (uint32_t)hl1_var_weather(seed, chain, y, years, V.n_weather, V.pick) * (uint32_t)H; }
                const uint32_t oi = wb * (uint32_t)nres + (uint32_t)h;            // out[(w * n_res + r) * H + h], r = 0
                double o0 = 0.0, o1 = 0.0;
                if (nres > 0) o0 = rout[oi];                                      // wave-uniform tests
                if (nres > 1) o1 = rout[oi + (uint32_t)H];
                {
                    uint32_t li = ((wb * (uint32_t)na) & lmask) + (uint32_t)h;    // lcurve[(w * na + a) * H + h], a = 0
                    for (int a = 0; a < na; ++a, li += (uint32_t)H) mg[a * 64] = hl1_storage_load(V.lscale[a], lcurve[li], V.lshift[a]);
                }
                // area a's close-out: its resources r ascending, then m_a = cap_a - L_a in L_a's slot
                const auto close_out = [&](int a, double cap) -> bool {
#pragma unroll
                    for (int r = 0; r < RELMC_HL1_VAR_MAX_RESOURCES; ++r)
                        if (r < nres && V.rarea[r] == a) {                        // wave-uniform
                            const double o = r == 0 ? o0 : r == 1 ? o1 : rout[oi + (uint32_t)r * (uint32_t)H];
                            cap = hl1_var_add(cap, V.rscale[r], o);
                        }
                    const double m = cap - mg[a * 64];
                    mg[a * 64] = m;
                    return m < 0.0;
                };
                int a = 0, kend = A->lo[1];                  // area a's units end at kend (every area has one unit at least)
                double cap = 0.0;
                bool neg = false;
                for (int q = 0; q < nw; ++q) {
                    const uint32_t up = ~seg[q][i];
                    const int kn = ngen - 32 * q < 32 ? ngen - 32 * q : 32;
                    for (int b = 0; b < kn; ++b) {
                        const int k = 32 * q + b;
                        if (k == kend) {
                            neg |= close_out(a, cap);
                            cap = 0.0; ++a; kend = A->lo[a + 1];
                        }
                        cap += ((up >> b) & 1u) ? A->cap[k] : 0.0;                    // ascending units; + 0.0 is exact
                    }
                }
                neg |= close_out(a, cap);
                if constexpr (TIES) {
                    if (inter && neg) {
                        const uint32_t tdown = seg[nw][i];
                        if (tdown) { area_tie_residual(R, TL, na, tdown); area_solve<false>(mg, R, nullptr, na, flow); }
                        else area_solve(mg, R, A->tie, na, flow);
                    }
                } else if (inter && neg) area_solve(mg, R, A->tie, na, flow);
#pragma unroll
                for (int r = 0; r < AREA_MAX; ++r) {
                    if (r >= na) break;
                    const double m = mg[r * 64];
                    if (m < 0.0) sw |= 1u << r;
                    if (stor && m > 0.0) lw |= 1u << r;
                }
            }
            if (__ballot(sw != 0u) != 0ull || (bits >> 8) != 0u) {               // wave-uniform; a quiet group does nothing
                uint32_t fw = sw;                            // bit a: a deficit is left in area a after the storages; bit na: in any
                if (stor) {
                    for (int r = 0; r < na; ++r) xyw[r * 64 + lane] = 0.0;
                    hl1_seq_wave_sync();                     // the lanes' margins and zeros, before the wave reads them step by step
                    int z = 0;
                    __asm__ volatile("" : "+s"(z));
                    uint64_t rest = ~0ull;                   // the steps after the one just visited
                    for (;;) {
                        const uint32_t can = area_var_can(V, ns, bits);
                        const uint64_t todo = __ballot(valid && ((sw & can) | (lw & (can >> 16))) != 0u) & rest;
                        if (todo == 0) break;
                        const int j = __builtin_ctzll(todo);
                        rest = j == 63 ? 0ull : ~0ull << (j + 1);
                        area_var_storage_step(V, ns, z, lane, j, mgw, xyw, soc, bits);
                    }
                    hl1_seq_wave_sync();
                    fw = 0u;
                    if (valid) {
#pragma unroll
                        for (int r = 0; r < AREA_MAX; ++r) {
                            if (r >= na) break;
                            if (((sw >> r) & 1u) && mg[r * 64] < 0.0) fw |= 1u << r;
                        }
                    }
                }
                uint32_t sv = sw & ~fw;                      // bit a: area a was short after the transfers and is served; bit na: the system
                if (sw != 0u && fw == 0u) sv |= 1u << na;
                if (fw) fw |= 1u << na;
                const uint32_t fl = (uint32_t)__shfl_up((int)fw, 1);
                const uint32_t rise = fw & ~(lane == 0 ? prev : fl);
                prev = (uint32_t)__shfl((int)fw, 63);
                for (;;) {
                    const bool in = valid && y == ycur;
                    if (in) {
                        double ds = 0.0, dd = 0.0, dc = 0.0;
                        for (int r = 0; r < na; ++r) {
                            const double mr_ = mg[r * 64];
                            const double c = ((fw >> r) & 1u) ? -mr_ : 0.0;
                            aE[r * 64] += c; ds += c;                // the system's deficit: sum of c_a in area order
                            if (stor) {
                                const double xy = xyw[r * 64 + lane];
                                const bool shr = (sw >> r) & 1u;
                                const double xd = shr ? xy : 0.0, xc = shr ? 0.0 : xy;
                                aD[r * 64] += xd; aC[r * 64] += xc; dd += xd; dc += xc;
                            }
                        }
                        aE[na * 64] += ds;
                        if (stor) { aD[na * 64] += dd; aC[na * 64] += dc; }
                    }
#pragma unroll
                    for (int r = 0; r <= AREA_MAX; ++r) {                   // a constant trip count: fully unrolled, the counts stay in registers
                        if (r <= na) {
                            cL[r] += (int)__popcll(__ballot(in && ((fw >> r) & 1u)));
                            cF[r] += (int)__popcll(__ballot(in && ((rise >> r) & 1u)));
                            if (stor) cS[r] += (int)__popcll(__ballot(in && ((sv >> r) & 1u)));
                        }
                    }
                    if (!__any(valid && y > ycur)) break;
#pragma unroll
                    for (int r = 0; r <= AREA_MAX; ++r)
                        if (r <= na) close(r);
                    ++ycur;
                }
            } else prev = 0u;
            gh += 64;
            while (gh >= H) { gh -= H; ++gy; }
        }
        hl1_seq_wave_sync();
    }
    for (; ycur < years; ++ycur) {
#pragma unroll
        for (int r = 0; r <= AREA_MAX; ++r)
            if (r <= na) close(r);
    }
}
}  // namespace relmc
