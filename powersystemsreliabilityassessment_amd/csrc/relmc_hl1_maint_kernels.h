// relmc_hl1_maint_kernels.h — planned maintenance on the HL1 sequential chronology (relmc_hl1_maint_seq, contract in include/relmc.h):
// one walk of a chain's fleet history compared with up to RELMC_HL1_MAINT_MAX_SCHEDULES maintenance schedules.  A unit on maintenance
// under schedule j in an hour adds 0.0 to that hour's capacity of schedule j; its failure and repair process runs on.
// An extension beyond the reference (generating_adequancy_comparative.jl has the overlay rule, on independently drawn hours).
#pragma once
#include <type_traits>
#include <utility>
#include "../../include/relmc.h"
#include "relmc_devfn.h"
#include "relmc_hl1_chrono.h"

namespace relmc {

// f(integral_constant<int, j>) for j = 0 .. NS - 1, written out at compile time: a schedule's registers are named by a constant
template <class F, int... J>
DEVFI void hl1_maint_each(F&& f, std::integer_sequence<int, J...>) { (f(std::integral_constant<int, J>{}), ...); }
template <int NS, class F>
DEVFI void hl1_maint_schedules(F&& f) { hl1_maint_each(f, std::make_integer_sequence<int, NS>{}); }

// The wave's open year of every schedule: loss hours and events are wave-uniform counts, schedule j's in lane j of cL / cF; EUE is the
// sequential model's fixed-order butterfly over the lanes' partials, skipped for a schedule without a loss hour in the year, whose
// partials are all +0.0 and sum to +0.0 in any order.  Lane 0 stores (lole, eue, lolf) at out + j * stride; the counts and partials
// restart at zero.
template <int NS>
DEVFI void hl1_maint_close_year(int ns, uint32_t& cL, uint32_t& cF, double (&aE)[NS], double* __restrict__ out, size_t stride)
{
    hl1_maint_schedules<NS>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        if (j < ns) {                                        // wave-uniform
            const uint32_t l = (uint32_t)__builtin_amdgcn_readlane((int)cL, j), f = (uint32_t)__builtin_amdgcn_readlane((int)cF, j);
            double e = 0.0;
            if (l != 0u) {                                   // wave-uniform
                e = aE[j];
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) e += __shfl_xor(e, off);
                aE[j] = 0.0;
            }
            if ((threadIdx.x & 63) == 0) { double* const o = out + (size_t)j * stride; o[0] = (double)l; o[1] = e; o[2] = (double)f; }
        }
    });
    cL = 0u; cF = 0u;
}

// Chain c = blockIdx.x * 4 + wave; the mapping, the cursors, the window fill and the step index are relmc_hl1_seq_kernel's (lane l owns
// units l and l + 64, cursors in registers, the down intervals of HL1_SEQ_WINDOW steps filled into the wave's LDS masks, one step per lane,
// no workgroup barrier).  The window loop is written out here and not shared as a function with the other tracks: relmc_hl1_chain_kernels.h
// says what the two attempts to share it cost the sequential model.
//
// tab[schedule][hour of the year][4]: bit k & 31 of word k >> 5 = unit k on maintenance.  The table holds NS schedules (the host adds
// empty ones above n_sched) and no bit at or above ngen.  Per step the lane reads its hour's words of each schedule -- consecutive lanes
// read consecutive hours, 16 bytes apart, so a wave's read of a schedule is one contiguous kilobyte -- and forms cap_j for the NS
// schedules in ONE ascending loop over the units: a unit's capacity is one scalar load for all schedules, and unit k adds cap_k to cap_j
// where its bit of (UP & ~maintenance_j) is set, 0.0 elsewhere.  With more than one schedule a first pass over the words asks whether any
// lane of the group has an UP unit on maintenance under any schedule; if none has, every cap_j is the one sum over the UP units (a unit
// that is DOWN adds 0.0 with or without maintenance, so the bits are those of the ascending sum).
// From there on it is the sweep's stage with schedules in place of levels: a first pass forms only the ballots of the loss flags, a group
// in which no schedule has a loss step and no schedule's flag was up on the step before does nothing further; otherwise each such
// schedule takes loss hours and rising edges by popcount of the ballots restricted to the lanes of the open year, the deficit into the
// lane's fp64 partial of the schedule, and its bit of the wave-uniform previous-step mask.  Years are closed when a later year shows up
// in an active group, or at the end of the chain.  The passes over the schedules are written out at compile time, so no register array is
// indexed at run time.  Records: year_out[schedule][chain of the launch][year][3].
template <int NS>
__global__ void __launch_bounds__(256) relmc_hl1_maint_kernel(const Hl1SeqCase* __restrict__ S, const double* __restrict__ load, uint64_t seed,
                                                              uint64_t first_chain, int64_t n_chains, int32_t years, int32_t start, double scale,
                                                              double shift, int32_t n_sched, const uint32_t* __restrict__ tab,
                                                              double* __restrict__ year_out)
{
    constexpr int W = HL1_SEQ_WINDOW;
    __shared__ uint32_t masks[4][4][W];                     // [wave][mask word][step of the window], bit k & 31 of word k >> 5 = unit k down
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t cl = (int64_t)blockIdx.x * 4 + wv;
    if (cl >= n_chains) return;                              // wave-uniform
    const uint64_t chain = first_chain + (uint64_t)cl;
    const int ngen = S->ngen, H = S->nhours, nw = (ngen + 31) >> 5, nslot = ngen > 64 ? 2 : 1;
    const int ns = n_sched < NS ? n_sched : NS;
    uint32_t (*const seg)[W] = masks[wv];
    const int64_t nsteps = (int64_t)years * H;
    const size_t stride = (size_t)n_chains * (size_t)years * 3;
    double* const out = year_out + (size_t)cl * (size_t)years * 3;      // the chain's year records of schedule 0

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

    double aE[NS];                                           // this lane's EUE partial of the open year ycur, per schedule
    hl1_maint_schedules<NS>([&](auto jc) { aE[decltype(jc)::value] = 0.0; });
    uint32_t cL = 0u, cF = 0u;                               // the wave's loss hours and loss events of the open year: schedule j's in lane j
    int ycur = 0;
    int gy = 0, gh = 0;                                      // chain year and hour of the year of the current 64-step group's first step
    uint32_t prevs = 0u;                                     // bit j: schedule j's loss flag on the step before the group (wave-uniform)
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
            int h = gh + lane, y = gy;                       // the step's hour of the year (< H, also in a lane without a step) and chain year
            while (h >= H) { h -= H; ++y; }
            const uint32_t* const mrow = tab + (size_t)h * 4;                     // schedule j's words of the hour: mrow[j * H * 4 + q]
            const size_t sched_words = (size_t)H * 4;
            double cap[NS];
            hl1_maint_schedules<NS>([&](auto jc) { cap[decltype(jc)::value] = 0.0; });
            bool overlay = true;                             // wave-uniform: some lane has an UP unit on maintenance under some schedule
            if constexpr (NS > 1) {
                uint32_t hit = 0u;
                for (int q = 0; q < nw; ++q) {
                    const uint32_t up = ~seg[q][i];
                    hl1_maint_schedules<NS>([&](auto jc) { hit |= up & mrow[(size_t)decltype(jc)::value * sched_words + q]; });
                }
                overlay = __builtin_amdgcn_ballot_w64(valid && hit != 0u) != 0;
            }
            if (overlay) {
                for (int q = 0; q < nw; ++q) {
                    const uint32_t up = ~seg[q][i];
                    uint32_t on[NS];                         // UP and not on maintenance under schedule j
                    hl1_maint_schedules<NS>([&](auto jc) {
                        constexpr int j = decltype(jc)::value;
                        on[j] = up & ~mrow[(size_t)j * sched_words + q];
                    });
                    const int kn = ngen - 32 * q < 32 ? ngen - 32 * q : 32;
                    for (int b = 0; b < kn; ++b) {
                        const double c = S->cap[32 * q + b];
                        hl1_maint_schedules<NS>([&](auto jc) {                    // ascending units; + 0.0 is exact
                            constexpr int j = decltype(jc)::value;
                            cap[j] += ((on[j] >> b) & 1u) ? c : 0.0;
                        });
                    }
                }
            } else {
                double all = 0.0;
                for (int q = 0; q < nw; ++q) {
                    const uint32_t up = ~seg[q][i];
                    const int kn = ngen - 32 * q < 32 ? ngen - 32 * q : 32;
                    for (int b = 0; b < kn; ++b) all += ((up >> b) & 1u) ? S->cap[32 * q + b] : 0.0;
                }
                hl1_maint_schedules<NS>([&](auto jc) { cap[decltype(jc)::value] = all; });
            }
            const double L = hl1_sweep_load(scale, load[h], shift);
            // which schedules have a loss step in the group (the comparison's lane mask is the ballot)
            uint32_t act = prevs;
            hl1_maint_schedules<NS>([&](auto jc) {
                constexpr int j = decltype(jc)::value;
                if (j < ns && __builtin_amdgcn_ballot_w64(valid && cap[j] < L) != 0) act |= 1u << j;
            });
            if (act != 0u) {                                 // wave-uniform
                uint32_t next = 0u;
                for (;;) {
                    const bool in = valid && y == ycur;
                    const uint64_t my = __builtin_amdgcn_ballot_w64(in);
                    next = 0u;
                    hl1_maint_schedules<NS>([&](auto jc) {
                        constexpr int j = decltype(jc)::value;
                        if ((act >> j) & 1u) {               // wave-uniform: a schedule without a loss step and without an open flag is left out
                            const bool fj = valid && cap[j] < L;
                            const uint64_t m = __builtin_amdgcn_ballot_w64(fj);
                            const uint64_t r = m & ~((m << 1) | (uint64_t)((prevs >> j) & 1u));     // the flag rises: the step before had none
                            cL += lane == j ? (uint32_t)__popcll(m & my) : 0u; cF += lane == j ? (uint32_t)__popcll(r & my) : 0u;
                            aE[j] += (fj && in) ? L - cap[j] : 0.0;
                            next |= (uint32_t)(m >> 63) << j;
                        }
                    });
                    if (!__any(valid && y > ycur)) break;
                    hl1_maint_close_year<NS>(ns, cL, cF, aE, out + (size_t)ycur * 3, stride);
                    ++ycur;
                }
                prevs = next;
            }
            gh += 64;
            while (gh >= H) { gh -= H; ++gy; }
        }
        hl1_seq_wave_sync();
    }
    for (; ycur < years; ++ycur) hl1_maint_close_year<NS>(ns, cL, cF, aE, out + (size_t)ycur * 3, stride);
}

}  // namespace relmc
