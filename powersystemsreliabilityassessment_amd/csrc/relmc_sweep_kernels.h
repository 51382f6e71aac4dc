// relmc_sweep_kernels.h — load sweep on the HL1 sequential chronology (relmc_hl1_seq_sweep, contract in include/relmc.h): one walk of a
// chain's fleet history compared with up to RELMC_HL1_SWEEP_MAX_LEVELS load levels L_j(h) = scale_j * load[h] + shift_j, each against the
// whole fleet or the fleet without the withheld units.  An extension beyond the reference (PowerSystemAdequacy.jl has one load curve).
#pragma once
#include <utility>
#include "../../include/relmc.h"
#include "relmc_devfn.h"
#include "relmc_hl1_chrono.h"

namespace relmc {

// The levels and the withheld-unit mask, passed BY VALUE as a kernel argument: every read of a level is a scalar load from the kernel
// argument segment, and the per-level branches are wave-uniform
struct Hl1SweepArgs {
    relmc_hl1_sweep_level lv[RELMC_HL1_SWEEP_MAX_LEVELS];
    uint32_t withheld[4];                                    // bit k & 31 of word k >> 5: unit k is not part of fleet 1
    int32_t n_levels;
    uint32_t fleet1;                                         // bit j: level j uses fleet 1 (lv[j].fleet, gathered by the host)
};
// The host fills lv[n_levels ..] with levels that never lose (scale 0, shift -inf: L = -inf, and no capacity is below it), so the passes
// over the levels need no test against n_levels; only the year records are written for j < n_levels alone.

// f(integral_constant<int, j>) for j = 0 .. NL - 1, written out at compile time: a level's registers are named by a constant.  (A
// `#pragma unroll` loop with the run-time exit at n_levels was left a loop at NL = 16, and the partials were then indexed at run time.)
template <class F, int... J>
DEVFI void hl1_sweep_each(F&& f, std::integer_sequence<int, J...>) { (f(std::integral_constant<int, J>{}), ...); }
template <int NL, class F>
DEVFI void hl1_sweep_levels(F&& f) { hl1_sweep_each(f, std::make_integer_sequence<int, NL>{}); }

// L_j(h) = scale * load + shift with the product and the sum each rounded, as numpy's scale * load + shift (the contract's __dmul_rn /
// __dadd_rn: those two are plain operators in the HIP headers and were fused into one v_fma_f64 here, so the rule is stated to the compiler)
DEVFI double hl1_sweep_load(double scale, double ld, double shift)
{
#pragma clang fp contract(off)
    const double p = scale * ld;
    return p + shift;
}

// The wave's open year of every level: loss hours and events are wave-uniform counts, level j's in lane j of cL / cF (32 scalar registers
// as arrays: 391 scalar spills at 16 levels); EUE is relmc_hl1_seq_kernel's fixed-order butterfly
// over the lanes' partials (hl1_seq_close_year) -- skipped for a level without a loss hour in the year, whose partials are all +0.0 and
// sum to +0.0 in any order.  Lane 0 stores (lole, eue, lolf) at out + j * level_stride; the counts and partials restart at zero.
template <int NL>
DEVFI void hl1_sweep_close_year(int nl, uint32_t& cL, uint32_t& cF, double (&aE)[NL], double* __restrict__ out, size_t level_stride)
{
    hl1_sweep_levels<NL>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        if (j < nl) {                                        // wave-uniform
            const uint32_t l = (uint32_t)__builtin_amdgcn_readlane((int)cL, j), f = (uint32_t)__builtin_amdgcn_readlane((int)cF, j);
            double e = 0.0;
            if (l != 0u) {                                   // wave-uniform
                e = aE[j];
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) e += __shfl_xor(e, off);
                aE[j] = 0.0;
            }
            if ((threadIdx.x & 63) == 0) { double* const o = out + (size_t)j * level_stride; o[0] = (double)l; o[1] = e; o[2] = (double)f; }
        }
    });
    cL = 0u; cF = 0u;
}

// Chain c = blockIdx.x * 4 + wave; the chronology is relmc_hl1_seq_kernel's, word for word (lane l owns units l and l + 64, windows of
// HL1_SEQ_WINDOW steps filled into the wave's LDS masks, one step per lane, no workgroup barrier).  The window loop below is a COPY of
// relmc_hl1_seq_kernel's (relmc_seq_kernels.h), on purpose: the two attempts to share that loop between kernels each cost the
// sequential kernel 1.6-3 %, and this kernel must leave relmc_hl1_seq_kernel's code as it is.
//
// Per step the lane forms cap0 (every UP unit) and, if a level uses fleet 1, cap1 (a withheld unit adds 0.0) in the one ascending loop
// over the mask bits.  A first pass over the levels forms only the ballots of the loss flags: a 64-step group in which no level has a
// loss step and no level's flag was up on the step before does nothing further (nearly all groups).  Otherwise each level that has a loss
// step or an open flag takes: loss hours and rising edges by popcount of the ballots restricted to the lanes of the open year, the
// deficit into the lane's fp64 partial of the level (relmc_hl1_seq_kernel's order: the lane's steps of the year ascending, + 0.0 left out),
// and its bit of the wave-uniform previous-step mask.  Years are closed when a later year shows up in an active group, or at the end of
// the chain; a skipped group adds nothing, so closing late changes no sum.  NL is the level count padded to 1, 4, 8 or 16; the passes over the
// levels are written out at compile time (hl1_sweep_levels), so no register array is indexed at run time.
// Records: year_out[level][chain of the launch][year][3].
template <int NL>
__global__ void __launch_bounds__(256) relmc_hl1_sweep_kernel(const Hl1SeqCase* __restrict__ S, const double* __restrict__ load, uint64_t seed,
                                                              uint64_t first_chain, int64_t n_chains, int32_t years, int32_t start,
                                                              const Hl1SweepArgs A, double* __restrict__ year_out)
{
    constexpr int W = HL1_SEQ_WINDOW;
    __shared__ uint32_t masks[4][4][W];                     // [wave][mask word][step of the window], bit k & 31 of word k >> 5 = unit k down
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t cl = (int64_t)blockIdx.x * 4 + wv;
    if (cl >= n_chains) return;                              // wave-uniform
    const uint64_t chain = first_chain + (uint64_t)cl;
    const int ngen = S->ngen, H = S->nhours, nw = (ngen + 31) >> 5, nslot = ngen > 64 ? 2 : 1;
    const int nl = A.n_levels < NL ? A.n_levels : NL;
    const bool use1 = A.fleet1 != 0u;
    uint32_t (*const seg)[W] = masks[wv];
    const int64_t nsteps = (int64_t)years * H;
    const size_t level_stride = (size_t)n_chains * (size_t)years * 3;
    double* const out = year_out + (size_t)cl * (size_t)years * 3;

    bool down[2], mine[2];
    double tn[2], mf[2], mr[2];
    int ev[2];
    int64_t since[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int k = lane + 64 * s;
        mine[s] = k < ngen;
        mf[s] = mine[s] ? S->mttf[k] : 1.0; mr[s] = mine[s] ? S->mttr[k] : 1.0;
        down[s] = false; ev[s] = 0; since[s] = 1; tn[s] = 0.0;
        if (mine[s]) {
            if (start == RELMC_HL1_START_STATIONARY) { down[s] = hl1_seq_u(chain, k, 0, seed) < S->q[k]; ev[s] = 1; }
            tn[s] = __dmul_rn(-(down[s] ? mr[s] : mf[s]), log(hl1_seq_u(chain, k, ev[s], seed)));    // T_1 (= 0 + duration)
            ++ev[s];
        }
    }

    double aE[NL];                                           // this lane's EUE partial of the open year ycur, per level
    uint32_t cL = 0u, cF = 0u;                               // the wave's loss hours and loss events of the open year: level j's in lane j
    hl1_sweep_levels<NL>([&](auto jc) { aE[decltype(jc)::value] = 0.0; });
    int ycur = 0, gy = 0, gh = 0;                            // gy / gh: chain year and hour of the current 64-step group's first step
    uint32_t prev = 0u;                                      // bit j: level j's loss flag on the step before the group (wave-uniform)
    for (int64_t w0 = 1; w0 <= nsteps; w0 += W) {
        const int64_t w1 = w0 + W;
        const int wlen = nsteps - w0 + 1 < W ? (int)(nsteps - w0 + 1) : W;
        for (int q = 0; q < nw; ++q)
            for (int i = lane; i < W; i += 64) seg[q][i] = 0u;
        hl1_seq_wave_sync();
        // (1) down intervals [ceil(T_odd), ceil(T_even)) of the window
#pragma unroll
        for (int s = 0; s < 2; ++s) {                        // unrolled: the cursors stay in registers
            if (s >= nslot) break;
            bool more = mine[s];
            while (__any(more)) {
                int fb = 0, fe = 0;
                if (more) {
                    const int64_t c = (int64_t)__builtin_ceil(tn[s]);             // the transition takes effect from step c on
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
                    uint32_t* const row = seg[sk >> 5];
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
            double cap0 = 0.0, cap1 = 0.0;
            if (!use1) {                                     // wave-uniform
                for (int q = 0; q < nw; ++q) {
                    const uint32_t up = ~seg[q][i];
                    const int kn = ngen - 32 * q < 32 ? ngen - 32 * q : 32;
                    for (int b = 0; b < kn; ++b) cap0 += ((up >> b) & 1u) ? S->cap[32 * q + b] : 0.0;   // ascending units; + 0.0 is exact
                }
            } else {
                for (int q = 0; q < nw; ++q) {
                    const uint32_t up = ~seg[q][i], wh = A.withheld[q];
                    const int kn = ngen - 32 * q < 32 ? ngen - 32 * q : 32;
                    for (int b = 0; b < kn; ++b) {
                        const double c = S->cap[32 * q + b], c1 = ((wh >> b) & 1u) ? 0.0 : c;          // a withheld unit adds 0.0
                        cap0 += ((up >> b) & 1u) ? c : 0.0;
                        cap1 += ((up >> b) & 1u) ? c1 : 0.0;
                    }
                }
            }
            const double ld = load[h];
            // which levels have a loss step in the group (the comparison's lane mask is the ballot)
            uint32_t act = prev;
            // a level's scale, shift and fleet bit are read where they are used (z is a zero the compiler cannot see through): read once
            // before the loops they are some 100 scalar registers live across the whole chain, most of them spilled to vector lanes
            int z = 0;
            __asm__ volatile("" : "+s"(z));
            const uint32_t fleet1 = A.fleet1 | (uint32_t)z;
            hl1_sweep_levels<NL>([&](auto jc) {
                constexpr int j = decltype(jc)::value;
                const double L = hl1_sweep_load(A.lv[j + z].scale, ld, A.lv[j + z].shift);
                const double cap = ((fleet1 >> j) & 1u) ? cap1 : cap0;
                if (__builtin_amdgcn_ballot_w64(valid && cap < L) != 0) act |= 1u << j;
            });
            if (act != 0u) {                                 // wave-uniform
                // the levels' loads and flags are formed again from a copy of the load the compiler cannot see through: kept from the
                // pass above they are 16 loads and 16 lane masks live across every group (167 vector registers, 323 scalar spills)
                double lda = ld;
                __asm__ volatile("" : "+v"(lda));
                uint32_t next = 0u;
                for (;;) {
                    const bool in = valid && y == ycur;
                    const uint64_t my = __builtin_amdgcn_ballot_w64(in);
                    next = 0u;
                    hl1_sweep_levels<NL>([&](auto jc) {
                        constexpr int j = decltype(jc)::value;
                        if ((act >> j) & 1u) {               // wave-uniform: a level without a loss step and without an open flag is left out
                            const double L = hl1_sweep_load(A.lv[j + z].scale, lda, A.lv[j + z].shift);
                            const double cap = ((fleet1 >> j) & 1u) ? cap1 : cap0;
                            const bool f = valid && cap < L;
                            const uint64_t m = __builtin_amdgcn_ballot_w64(f);
                            const uint64_t r = m & ~((m << 1) | (uint64_t)((prev >> j) & 1u));     // the flag rises: the step before had none
                            cL += lane == j ? (uint32_t)__popcll(m & my) : 0u; cF += lane == j ? (uint32_t)__popcll(r & my) : 0u;
                            aE[j] += (f && in) ? L - cap : 0.0;
                            next |= (uint32_t)(m >> 63) << j;
                        }
                    });
                    if (!__any(valid && y > ycur)) break;
                    hl1_sweep_close_year<NL>(nl, cL, cF, aE, out + (size_t)ycur * 3, level_stride);
                    ++ycur;
                }
                prev = next;
            }
            gh += 64;
            while (gh >= H) { gh -= H; ++gy; }
        }
        hl1_seq_wave_sync();
    }
    for (; ycur < years; ++ycur) hl1_sweep_close_year<NL>(nl, cL, cF, aE, out + (size_t)ycur * 3, level_stride);
}
}  // namespace relmc
