// relmc_hl1_attr_kernels.h — loss attribution on the HL1 sequential chronology (relmc_hl1_attr_seq, contract in include/relmc.h): every
// loss step of a chain is charged to the units that are DOWN in it.  Included by relmc_attr.hip alone.
// The kernel has a window loop of its own, as the storage, multi-state and area kernels have (the chain kernels' window
// loop is not shared, and a fifth model of relmc_hl1_chain_kernels.h's template would have to leave the other four's code as it is).
// The chronology is relmc_hl1_seq's, from the same text: the cursors, the start rule, the window clear, the interval fill, the step
// index with its hour / year walk and the ascending capacity sum; the year records are kept as the sweep keeps those of one level
// (counts by popcount of the loss ballot, groups without a loss step skipped, the EUE partials closed by the sequential model's
// butterfly), which gives relmc_hl1_seq's year records bit for bit.  Nothing of relmc_hl1_chain_kernels.h is needed here.
#pragma once
#include "../../include/relmc.h"
#include "relmc_devfn.h"
#include "relmc_hl1_chrono.h"

namespace relmc {

// Lane `src`'s value (src wave-uniform) in scalar registers
DEVFI double hl1_attr_lane(double x, int src)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), src), __builtin_amdgcn_readlane(__double2loint(x), src));
}

// Chain c = blockIdx.x * 4 + wave; lane l owns units l and l + 64 (its cursors stay in registers for the whole chain).
// Stage (1) and the capacity sum of stage (2) are the sequential model's (relmc_hl1_chain_kernels.h), the load is L = scale * load[h] +
// shift, and the account of a group is the sweep's for one level.  The wave takes the ballot of the loss flags.  A group without a loss
// step adds nothing to the unit records (nearly all groups).  Otherwise the
// set bits are walked in ascending lane order, which is step order: the step's capacity and load come by readlane, its window index is
// wave-uniform, and every lane tests its own units' bits in the step's mask words (lanes 0..31 and lanes 32..63 each read one address:
// two broadcasts) and adds to its units' four accumulators.  The accumulators are the chain's unit records themselves, in global
// memory: zeroed at the chain's start, read at the head of a loss group and written back at its end by the one lane that owns the unit,
// so they cost no register outside a loss group, and a unit's fp64 sums are one accumulator each, added in ascending step order over
// the whole chain.  Lanes past the chain's last step carry no loss flag.
// Records: year_out[chain of the launch][year][3], unit_out[chain of the launch][unit][4] = (down_hours, down_mwh, critical_hours,
// relief_mwh); the counts are fp64 (steps of a chain: below 2^53).  No atomics.
__global__ void __launch_bounds__(256) relmc_hl1_attr_kernel(const Hl1SeqCase* __restrict__ S, const double* __restrict__ load, uint64_t seed,
                                                             uint64_t first_chain, int64_t n_chains, int32_t years, int32_t start,
                                                             double scale, double shift, double* __restrict__ year_out, double* __restrict__ unit_out)
{
    constexpr int W = HL1_SEQ_WINDOW;
    __shared__ uint32_t masks[4][4][W];                     // [wave][mask word][step of the window], bit k & 31 of word k >> 5 = unit k down
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t cl = (int64_t)blockIdx.x * 4 + wv;
    if (cl >= n_chains) return;                              // wave-uniform
    const uint64_t chain = first_chain + (uint64_t)cl;
    const int ngen = S->ngen, H = S->nhours, nw = (ngen + 31) >> 5, nslot = ngen > 64 ? 2 : 1;
    uint32_t (*const seg)[W] = masks[wv];
    const int64_t nsteps = (int64_t)years * H;
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
            double* const o = unit_out + ((size_t)cl * (size_t)ngen + (size_t)k) * 4;    // the unit's record of the chain starts at zero
            o[0] = 0.0; o[1] = 0.0; o[2] = 0.0; o[3] = 0.0;
        }
    }

    // The open year ycur, kept as the sweep keeps a level's: loss hours and loss events are wave-uniform counts (popcounts of the loss
    // ballot), the EUE a lane partial (the lane's steps of the year ascending, + 0.0 left out) closed by the sequential model's butterfly
    double aE = 0.0;
    uint32_t cL = 0u, cF = 0u;
    int ycur = 0, gy = 0, gh = 0;                            // open year; chain year and hour of the year of the group's first step
    bool prev = false;                                       // loss flag of the step before the group (none before step 1), wave-uniform
    // closes the open year: lane 0 stores (lole, eue, lolf); a year without a loss hour has partials that are all +0.0 and sum to +0.0
    auto close_year = [&]() {
        double e = 0.0;
        if (cL != 0u) {                                      // wave-uniform
            e = aE;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) e += __shfl_xor(e, off);
            aE = 0.0;
        }
        if (lane == 0) { double* const o = out + (size_t)ycur * 3; o[0] = (double)cL; o[1] = e; o[2] = (double)cF; }
        cL = 0u; cF = 0u;
        ++ycur;
    };
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
            int h = gh + lane, y = gy;                       // the step's hour of the year and chain year
            while (h >= H) { h -= H; ++y; }
            bool f = false;
            double cap = 0.0, L = 0.0;
            if (valid) {
                for (int q = 0; q < nw; ++q) {
                    const uint32_t up = ~seg[q][i];
                    const int kn = ngen - 32 * q < 32 ? ngen - 32 * q : 32;
                    for (int b = 0; b < kn; ++b) cap += ((up >> b) & 1u) ? S->cap[32 * q + b] : 0.0;   // ascending units; + 0.0 is exact
                }
                L = hl1_sweep_load(scale, load[h], shift);
                f = cap < L;
            }
            const uint64_t m = __ballot(f);                  // lanes past the chain's last step carry no loss
            // A group without a loss step whose predecessor step was none either adds nothing to any year (nearly all groups): years are
            // closed when a later year shows up in a group that counts, or at the chain's end, and closing late changes no sum
            if (m != 0 || prev) {                            // wave-uniform
                const uint64_t r = m & ~((m << 1) | (uint64_t)prev);                  // the flag rises: the step before had none
                for (;;) {
                    const bool in = valid && y == ycur;
                    const uint64_t my = __ballot(in);
                    cL += (uint32_t)__popcll(m & my); cF += (uint32_t)__popcll(r & my);
                    aE += (f && in) ? L - cap : 0.0;
                    if (!__any(valid && y > ycur)) break;
                    close_year();
                }
                prev = (m >> 63) != 0;
            }
            // the group's loss steps, in step order, charged to the units that are DOWN in them
            if (m != 0) {                                    // wave-uniform; nearly every group has none
                // the lane number as a value the compiler cannot see through: formed from `lane` ahead of the window loop, the addresses
                // below are vector registers live across the whole chain, and with them the kernel loses the sequential model's occupancy
                int ln = lane;
                __asm__ volatile("" : "+v"(ln));
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    if (s >= nslot) break;
                    if (mine[s]) {
                        // unit k = lane + 64 s: bit lane & 31 of word 2 s + (lane >> 5), a word below nw
                        const uint32_t* const word = seg[2 * s + (ln >> 5)];
                        double* const o = unit_out + ((size_t)cl * (size_t)ngen + (size_t)(ln + 64 * s)) * 4;
                        const double ck = S->cap[ln + 64 * s];
                        // two passes over the group's loss steps, each with one fp64 sum and one count of at most 64, so that few values
                        // are live beside cap and L (one pass with four fp64 accumulators and the deficit kept from the step stage was 102
                        // vector registers, one wave per SIMD less, while the year records were still lane partials).  The step's deficit
                        // is formed again from its capacity and load, the same difference with the same bits
                        {
                            double uE = o[1];
                            int nH = 0;
                            for (uint64_t mm = m; mm; mm &= mm - 1) {             // ascending lanes = step order
                                const int src = __builtin_ctzll(mm);              // the step's lane; its window index g + src is below wlen
                                const double ds = hl1_attr_lane(L, src) - hl1_attr_lane(cap, src);
                                if ((word[g + src] >> (ln & 31)) & 1u) { ++nH; uE += ds; }
                            }
                            o[0] += (double)nH; o[1] = uE;
                        }
                        {
                            double uR = o[3];
                            int nC = 0;
                            for (uint64_t mm = m; mm; mm &= mm - 1) {
                                const int src = __builtin_ctzll(mm);
                                const double cs = hl1_attr_lane(cap, src), Ls = hl1_attr_lane(L, src), ds = Ls - cs;
                                if ((word[g + src] >> (ln & 31)) & 1u) {
                                    nC += !(cs + ck < Ls) ? 1 : 0;                // with k UP the step is no loss step; a tie counts
                                    uR += fmin(ds, ck);
                                }
                            }
                            o[2] += (double)nC; o[3] = uR;
                        }
                    }
                }
            }
            gh += 64;
            while (gh >= H) { gh -= H; ++gy; }
        }
        hl1_seq_wave_sync();
    }
    while (ycur < years) close_year();
}

// Sums of relmc_hl1_attr_acc over the n chain records of one launch, rec[chain][ngen][4]: workgroup (k, b) of a (ngen, B) grid takes
// unit k and the chains b * 256 + t, + B * 256, ... (grid-stride in a fixed order), then a fixed tree; partial[b][k][8] = (sum[4], sum2[4])
__global__ void __launch_bounds__(256) relmc_hl1_attr_reduce_kernel(const double* __restrict__ rec, int64_t n, int32_t ngen, double* __restrict__ partial)
{
    __shared__ double red[8][256];
    const int tid = threadIdx.x, k = blockIdx.x;
    double s[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t c = (int64_t)blockIdx.y * 256 + tid; c < n; c += (int64_t)gridDim.y * 256) {
        const double* const x = rec + ((size_t)c * (size_t)ngen + (size_t)k) * 4;
#pragma unroll
        for (int j = 0; j < 4; ++j) { const double v = x[j]; s[j] += v; s[4 + j] = __builtin_fma(v, v, s[4 + j]); }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) red[j][tid] = s[j];
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off) {
#pragma unroll
            for (int j = 0; j < 8; ++j) red[j][tid] += red[j][tid + off];
        }
        __syncthreads();
    }
    if (tid < 8) partial[((size_t)blockIdx.y * (size_t)ngen + (size_t)k) * 8 + tid] = red[tid][0];
}

}  // namespace relmc
