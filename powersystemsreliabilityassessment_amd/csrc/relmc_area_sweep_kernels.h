// relmc_area_sweep_kernels.h — sweep of the HL1 multi-area chronology (relmc_hl1_area_sweep, contract in include/relmc.h): one walk of a
// chain's unit and tie history against up to RELMC_HL1_AREA_SWEEP_MAX_LEVELS levels, each with its own load curves (scale and shift per
// area), tie capacities and fleet (every unit, or the fleet without the withheld units).  An extension beyond the reference
// (AdequacyAssessmentII.jl evaluates one system per run).
#pragma once
#include "relmc_area_kernels.h"

namespace relmc {

// Each area's capacity of one step, once per fleet in use: fleet 0 (every UP unit) to c0[a] and, with F1, fleet 1 (a withheld unit adds
// 0.0) to c1[a], each from 0.0 over the area's units in ascending order as relmc_hl1_area_kernel sums them; the areas' loads of hour h to
// ld[a].  The loop over the areas is written out (a is a constant in every body), so the three arrays are registers.
template <bool F1>
DEVFI void area_sweep_caps(const AreaCase* __restrict__ A, const uint32_t* __restrict__ withheld, const uint32_t (*__restrict__ seg)[HL1_SEQ_WINDOW],
                           const double* __restrict__ load, int i, int h, int na, int H, double (&c0)[AREA_MAX], double (&c1)[AREA_MAX],
                           double (&ld)[AREA_MAX])
{
#pragma unroll
    for (int a = 0; a < AREA_MAX; ++a) {
        if (a >= na) break;                                  // wave-uniform
        const int k0 = A->lo[a], k1 = A->lo[a + 1];
        double s0 = 0.0, s1 = 0.0;
        for (int q = k0 >> 5; 32 * q < k1; ++q) {
            const uint32_t up = ~seg[q][i], wh = F1 ? withheld[q] : 0u;
            const int b0 = k0 > 32 * q ? k0 - 32 * q : 0, b1 = k1 - 32 * q < 32 ? k1 - 32 * q : 32;
            for (int b = b0; b < b1; ++b) {
                const double c = A->cap[32 * q + b];
                s0 += ((up >> b) & 1u) ? c : 0.0;            // ascending units; + 0.0 is exact
                if constexpr (F1) s1 += ((up >> b) & 1u) ? (((wh >> b) & 1u) ? 0.0 : c) : 0.0;
            }
        }
        c0[a] = s0; c1[a] = s1;
        ld[a] = load[(size_t)a * H + h];
    }
}

// The open year of one level: relmc_hl1_area_kernel's fixed-order butterfly over the lanes' EUE partials aE[r * 64] of every row r --
// skipped for a row without a loss hour in the year, whose partials are all +0.0 and sum to +0.0 in any order -- then lane r stores row
// r's (loss hours, EUE, loss events) at out + r * row_stride.  The level's counts (row r's in lane base + r of cL / cF) and the partials
// restart at zero.
DEVFI void area_sweep_close_year(double* __restrict__ aE, uint32_t& cL, uint32_t& cF, int base, int na, double* __restrict__ out, size_t row_stride)
{
    const int lane = threadIdx.x;
    double myE = 0.0;
    uint32_t myL = 0u, myF = 0u;
    for (int r = 0; r <= na; ++r) {
        const uint32_t l = (uint32_t)__builtin_amdgcn_readlane((int)cL, base + r), f = (uint32_t)__builtin_amdgcn_readlane((int)cF, base + r);
        if (l != 0u) {                                       // wave-uniform
            double e = aE[r * 64];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) e += __shfl_xor(e, off);
            aE[r * 64] = 0.0;
            myE = lane == r ? e : myE; myL = lane == r ? l : myL; myF = lane == r ? f : myF;
        }
    }
    if (lane <= na) { double* const o = out + (size_t)lane * row_stride; o[0] = (double)myL; o[1] = myE; o[2] = (double)myF; }
    const bool mine = lane >= base && lane < base + 16;
    cL = mine ? 0u : cL; cF = mine ? 0u : cF;
}

// One 64-step group of one level after its solve: relmc_hl1_area_kernel's counts and lane partials of the level's open year yj, the
// years closed as later ones show up in the group.  mg: the lane's margins after the solve; fw / rise: its loss mask and rising edges.
DEVFI void area_sweep_account(bool valid, int y, uint32_t fw, uint32_t rise, const double* __restrict__ mg, double* __restrict__ aE, int na,
                              uint32_t& cL, uint32_t& cF, int base, int& yj, double* __restrict__ out, size_t row_stride)
{
    const int lane = threadIdx.x;
    for (;;) {
        const bool in = valid && y == yj;
        if (in && fw) {
            double ds = 0.0;
            for (int r = 0; r < na; ++r) {
                const double mr_ = mg[r * 64];
                const double c = mr_ < 0.0 ? -mr_ : 0.0;
                aE[r * 64] += c; ds += c;                    // the system's deficit: sum of c_a in area order
            }
            aE[na * 64] += ds;
        }
        for (int r = 0; r <= na; ++r) {
            const uint32_t pl = (uint32_t)__popcll(__ballot(in && ((fw >> r) & 1u)));
            const uint32_t pf = (uint32_t)__popcll(__ballot(in && ((rise >> r) & 1u)));
            cL += lane == base + r ? pl : 0u; cF += lane == base + r ? pf : 0u;
        }
        if (!__any(valid && y > yj)) break;
        area_sweep_close_year(aE, cL, cF, base, na, out + (size_t)yj * 3, row_stride);
        ++yj;
    }
}

// Chain c = first_chain + blockIdx.x: one wavefront per workgroup, one chain per wavefront, as relmc_hl1_area_kernel.  The window loop
// below (the cursors of the units and, with TIES, of the ties; the window fill) is a COPY of that kernel's, on purpose: that kernel's code
// must stay as it is, and sharing a window loop between kernels has cost the older kernel 1.6-3 % twice (relmc_hl1_chain_kernels.h, DESIGN.md
// 6.12).
//
// Per step (one per lane): each area's capacity once per fleet in use and the areas' loads, in registers (area_sweep_caps).  Then the
// levels one after another on the same margin and residual scratch in LDS: the level's margins m_a = cap_fleet,a - (scale_a * load_a[h] +
// shift_a); a level without a negative margin in the whole 64-step group takes nothing further (its flags are all down: no hour, no
// event, no energy).  Otherwise the transfer solve where the lane's step has a negative margin -- left out for a level whose ties all
// have capacity 0, where it could move nothing -- from the level's all-UP matrix X->lv[j].tie, or with a tie DOWN from the level's UP
// ties (area_tie_residual with the level's capacities); then relmc_hl1_area_kernel's flags, rising edges, counts and lane partials (area_sweep_account).
//
// Per-level state is held where a run-time level index costs nothing: the EUE partials aE[(j * rows + r) * 64 + lane] in LDS; the open
// year and the previous-step loss mask of level j in lane j of two vector registers; the year's counts of level j, row r in lane
// (j & 3) * 16 + r of the register pair of levels 0-3 or of levels 4-7.  No register array is indexed by the level, so the level loop
// stays a loop and nothing goes to scratch (relmc_hl1_chain_kernels.h tells what happened otherwise).  A level's year is closed when the
// level next takes a group with a later year in it, or at the end of the chain; a group it left out added nothing, so closing late
// changes no sum.
// Dynamic LDS, in this order: aE [n_levels * rows][64], margins [na][64], residuals [na * na][64] (fp64), masks [nw (+ 1 with
// TIES)][HL1_SEQ_WINDOW] (u32).  Records: rec[level][row][chain * years + year][3], rows `stride` records apart.
template <bool TIES>
__global__ void __launch_bounds__(64) relmc_hl1_area_sweep_kernel(const AreaCase* __restrict__ A, const AreaTies* __restrict__ TL,
                                                                  const AreaSweepTab* __restrict__ X, const double* __restrict__ load,
                                                                  uint64_t seed, uint64_t first_chain, int32_t years, int32_t start,
                                                                  int32_t flow, int64_t stride, double* __restrict__ rec)
{
    constexpr int NS = TIES ? 3 : 2;                         // cursor slots per lane: units lane, lane + 64, and tie `lane`
    constexpr int W = HL1_SEQ_WINDOW;
    extern __shared__ double lds[];
    const int lane = threadIdx.x;
    const int64_t cl = blockIdx.x;
    const uint64_t chain = first_chain + (uint64_t)cl;
    const int ngen = A->ngen, H = A->nhours, na = A->n_areas, nw = (ngen + 31) >> 5, nslot = ngen > 64 ? 2 : 1;
    const int nl = X->n_levels, rows = na + 1;
    const uint32_t fleet1 = X->fleet1, solve = X->solve;
    double* const aE = lds + lane;
    double* const mg = lds + 64 * (nl * rows) + lane;
    double* const R = mg + 64 * na;
    uint32_t (*const seg)[W] = reinterpret_cast<uint32_t (*)[W]>(lds + 64 * (nl * rows + na + na * na));
    const int64_t nsteps = (int64_t)years * H;
    const size_t row_stride = (size_t)stride * 3, level_stride = row_stride * (size_t)rows;
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

    for (int e = 0; e < nl * rows; ++e) aE[e * 64] = 0.0;
    uint32_t cLa = 0u, cFa = 0u, cLb = 0u, cFb = 0u;         // loss hours / events of the open years: levels 0-3 (a) and 4-7 (b)
    int ycv = 0;                                             // lane j: the open year of level j
    uint32_t prevv = 0u;                                     // lane j: level j's loss mask of the step before the group (none before step 1)
    int gy = 0, gh = 0;
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
            uint32_t tdown = 0u;
            double c0[AREA_MAX], c1[AREA_MAX], ld[AREA_MAX];
#pragma unroll
            for (int a = 0; a < AREA_MAX; ++a) c0[a] = c1[a] = ld[a] = 0.0;
            if (valid) {
                if (fleet1 != 0u) area_sweep_caps<true>(A, X->withheld, seg, load, i, h, na, H, c0, c1, ld);   // wave-uniform
                else area_sweep_caps<false>(A, X->withheld, seg, load, i, h, na, H, c0, c1, ld);
                if constexpr (TIES) tdown = seg[nw][i];
            }
            for (int j = 0; j < nl; ++j) {
                const AreaSweepLevelTab* __restrict__ const Lj = &X->lv[j];
                const bool f1 = (fleet1 >> j) & 1u;          // wave-uniform
                bool neg = false;
#pragma unroll
                for (int a = 0; a < AREA_MAX; ++a) {
                    if (a >= na) break;
                    const double m = (f1 ? c1[a] : c0[a]) - hl1_sweep_load(Lj->scale[a], ld[a], Lj->shift[a]);
                    mg[a * 64] = m; neg |= valid && m < 0.0;
                }
                if (!__any(neg)) {                           // wave-uniform: every flag of the group is down
                    prevv = lane == j ? 0u : prevv;
                    continue;
                }
                uint32_t fw = 0u;
                if (neg) {
                    if ((solve >> j) & 1u) {
                        if constexpr (TIES) {
                            if (tdown) { area_tie_residual(R, TL, Lj->cap, na, tdown); area_solve<false>(mg, R, nullptr, na, flow); }
                            else area_solve(mg, R, Lj->tie, na, flow);
                        } else area_solve(mg, R, Lj->tie, na, flow);
                    }
#pragma unroll
                    for (int r = 0; r < AREA_MAX; ++r) {
                        if (r >= na) break;
                        if (mg[r * 64] < 0.0) fw |= 1u << r;
                    }
                    if (fw) fw |= 1u << na;
                }
                const uint32_t pj = (uint32_t)__builtin_amdgcn_readlane((int)prevv, j);
                const uint32_t fl = (uint32_t)__shfl_up((int)fw, 1);
                const uint32_t rise = fw & ~(lane == 0 ? pj : fl);
                const uint32_t last = (uint32_t)__shfl((int)fw, 63);
                prevv = lane == j ? last : prevv;
                int yj = __builtin_amdgcn_readlane(ycv, j);
                double* const aEj = aE + (size_t)(j * rows) * 64;
                double* const outj = out + (size_t)j * level_stride;
                if (j < 4) area_sweep_account(valid, y, fw, rise, mg, aEj, na, cLa, cFa, (j & 3) * 16, yj, outj, row_stride);   // wave-uniform
                else area_sweep_account(valid, y, fw, rise, mg, aEj, na, cLb, cFb, (j & 3) * 16, yj, outj, row_stride);
                ycv = lane == j ? yj : ycv;
            }
            gh += 64;
            while (gh >= H) { gh -= H; ++gy; }
        }
        hl1_seq_wave_sync();
    }
    for (int j = 0; j < nl; ++j)
        for (int yj = __builtin_amdgcn_readlane(ycv, j); yj < years; ++yj) {
            double* const aEj = aE + (size_t)(j * rows) * 64;
            double* const o = out + (size_t)j * level_stride + (size_t)yj * 3;
            if (j < 4) area_sweep_close_year(aEj, cLa, cFa, (j & 3) * 16, na, o, row_stride);
            else area_sweep_close_year(aEj, cLb, cFb, (j & 3) * 16, na, o, row_stride);
        }
}
}  // namespace relmc
