// relmc_multistate_kernels.h — the HL1 sequential chronology with three-state units (relmc_hl1_ms_seq, contract in include/relmc.h):
// every unit is a continuous-time Markov chain over UP / DERATED / DOWN, given by its mean holding times and the branch probabilities
// of its jumps.  An extension beyond the reference (its Markov_process.jl and PowerSystemAdequacy.jl:214-268 stop at two states).
#pragma once
#include "../../include/relmc.h"
#include "relmc_devfn.h"
#include "relmc_hl1_chrono.h"

namespace relmc {

// U of branch draw e of unit k in chain c: hl1_seq_u's stream under the tag RELMC_HL1_MS_BRANCH_TAG, which no other kernel uses
DEVFI double hl1_ms_branch_u(uint64_t chain, int k, int e, uint64_t seed)
{
    uint32_t w[4];
    philox4x32_10((uint32_t)chain, (uint32_t)(chain >> 32), (uint32_t)k | RELMC_HL1_MS_BRANCH_TAG, (uint32_t)e >> 2, (uint32_t)seed, (uint32_t)(seed >> 32), w);
    const uint32_t x = (e & 2) ? ((e & 1) ? w[3] : w[2]) : ((e & 1) ? w[1] : w[0]);      // selects, not a dynamic index into w (scratch)
    return ((double)x + 0.5) * 2.3283064365386963e-10;
}

// How each state of a unit picks its destination, two bits per state (state s at bits 2 s): 0 = always the other destination (first_p
// == 0), 1 = always the first-listed one (first_p == 1), 2 = by the branch draw.  The cursor keeps these six bits, not the three
// probabilities: a probability strictly inside (0, 1) is read from the case when its draw is made, behind the ten Philox rounds.
DEVFI uint32_t hl1_ms_kinds(double f0, double f1, double f2)
{
    const auto kd = [](double f) { return f >= 1.0 ? 1u : f <= 0.0 ? 0u : 2u; };
    return kd(f0) | (kd(f1) << 2) | (kd(f2) << 4);
}

// a value of the cursor's state (0 UP, 1 DERATED, 2 DOWN) as two selects: the three candidates stay in registers
DEVFI double hl1_ms_pick(int st, double v0, double v1, double v2) { return st == 0 ? v0 : st == 1 ? v1 : v2; }

// The wave's open year: relmc_hl1_seq_kernel's fixed-order butterfly (hl1_seq_close_year), widened by the two state counts; lane 0 stores
// (lole, eue, lolf) and (derated_unit_h, down_unit_h, 0); the partials restart at zero
DEVFI void hl1_ms_close_year(uint32_t& cl, double& e, uint32_t& cf, uint32_t& cd, uint32_t& cn, double* __restrict__ out0, double* __restrict__ out1)
{
    // a lane's counts of a year are at most 128 units x (nhours / 64 + 2) steps <= 2^31 + 256, since relmc_hl1_ms_load refuses
    // nhours > RELMC_HL1_MS_MAX_HOURS = 2^30: they fit 32 bits; the fleet's sums over the 64 lanes may not, and are formed in doubles
    double l = (double)cl, f = (double)cf, d = (double)cd, n = (double)cn;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        l += __shfl_xor(l, off); e += __shfl_xor(e, off); f += __shfl_xor(f, off);
        d += __shfl_xor(d, off); n += __shfl_xor(n, off);
    }
    if ((threadIdx.x & 63) == 0) { out0[0] = l; out0[1] = e; out0[2] = f; out1[0] = d; out1[1] = n; out1[2] = 0.0; }
    e = 0.0;
    cl = cf = cd = cn = 0u;
}

// Chain c = blockIdx.x * 4 + wave; the structure is relmc_hl1_seq_kernel's (lane l owns units l and l + 64, the cursors stay in
// registers, windows filled into the wave's LDS masks, one step per lane, no workgroup barrier).  The window loop below is a COPY of
// relmc_hl1_seq_kernel's (relmc_hl1_chain_kernels.h), on purpose: sharing that loop between kernels cost the sequential kernel 1.6-3 % twice
// (DESIGN.md 6.12).  What differs:
//   cursor    a state 0 / 1 / 2 instead of `down`, the unit's three means and how each state branches (hl1_ms_kinds); the transition
//             that ends the sojourn timed by duration draw e takes its destination from branch draw e (hl1_ms_branch_u), and only when
//             the branch probability lies strictly inside (0, 1): a two-state unit never pays for the second stream
//   window    HL1_MS_WINDOW = 256 steps with two bit planes per step, DERATED and DOWN (a unit is in at most one): the 8 KB per wave
//             of relmc_hl1_seq_kernel's one plane over 512 steps, so a CU holds as many waves.  A sojourn in state 1 or 2 is filled
//             into its plane by the whole wave, 64 steps per instruction; each lane touches its own step, so a plain OR is race-free
//   step      a unit adds derated_mw when its DERATED bit is set, 0.0 when its DOWN bit is set, capacity_mw otherwise, in ascending
//             unit order (the second select only for the units derated somewhere in the 64-step group); the two unit-hour counts are
//             the popcounts of the planes' words, masked to ngen
// Records: year_out[row][chain of the launch][year][3], row 0 = (lole, eue, lolf), row 1 = (derated_unit_h, down_unit_h, 0): three
// doubles per record in both rows, so that relmc_hl1_reduce_kernel sums either.
__global__ void __launch_bounds__(256) relmc_hl1_ms_kernel(const Hl1MsCase* __restrict__ S, const double* __restrict__ load, uint64_t seed,
                                                           uint64_t first_chain, int64_t n_chains, int32_t years, int32_t start,
                                                           double* __restrict__ year_out)
{
    constexpr int W = HL1_MS_WINDOW;
    __shared__ uint32_t masks[4][2][4][W];                  // [wave][plane: DERATED, DOWN][mask word][step of the window], bit k & 31 of word k >> 5 = unit k
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t cl = (int64_t)blockIdx.x * 4 + wv;
    if (cl >= n_chains) return;                              // wave-uniform
    const uint64_t chain = first_chain + (uint64_t)cl;
    const int ngen = S->ngen, H = S->nhours, nw = (ngen + 31) >> 5, nslot = ngen > 64 ? 2 : 1;
    uint32_t (*const seg)[4][W] = masks[wv];
    const int64_t nsteps = (int64_t)years * H;
    double* const out0 = year_out + (size_t)cl * (size_t)years * 3;
    double* const out1 = out0 + (size_t)n_chains * (size_t)years * 3;

    bool mine[2];
    int st[2], ev[2];
    double tn[2], m0[2], m1[2], m2[2];
    uint32_t kind[2];                                        // hl1_ms_kinds of the unit
    int since[2];                                            // the first step of the present sojourn, relative to the window's first (0: it began before)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int k = lane + 64 * s;
        mine[s] = k < ngen;
        m0[s] = mine[s] ? S->mean[0][k] : 1.0; m1[s] = mine[s] ? S->mean[1][k] : 1.0; m2[s] = mine[s] ? S->mean[2][k] : 1.0;
        kind[s] = mine[s] ? hl1_ms_kinds(S->first_p[0][k], S->first_p[1][k], S->first_p[2][k]) : 0x15u;
        st[s] = 0; ev[s] = 0; since[s] = 0; tn[s] = 0.0;
        if (mine[s]) {
            if (start == RELMC_HL1_START_STATIONARY) {
                const double u = hl1_seq_u(chain, k, 0, seed);
                st[s] = u < S->thr_down[k] ? 2 : u < S->thr_out[k] ? 1 : 0;
                ev[s] = 1;
            }
            tn[s] = __dmul_rn(-hl1_ms_pick(st[s], m0[s], m1[s], m2[s]), log(hl1_seq_u(chain, k, ev[s], seed)));    // T_1 (= 0 + duration)
            ++ev[s];
        }
    }

    double aE = 0.0;                                         // this lane's partials of the open year ycur: the EUE in relmc_hl1_seq_kernel's order,
    uint32_t aL = 0u, aF = 0u, aD = 0u, aN = 0u;             // the counts as integers (exact in any order; the butterfly adds them as doubles)
    int ycur = 0, gy = 0, gh = 0;                            // gy / gh: chain year and hour of the current 64-step group's first step
    bool prev = false;                                       // loss flag of the step before the group (none before step 1)
    for (int64_t w0 = 1; w0 <= nsteps; w0 += W) {
        const int64_t w1 = w0 + W;
        const int wlen = nsteps - w0 + 1 < W ? (int)(nsteps - w0 + 1) : W;
        for (int q = 0; q < nw; ++q)
            for (int i = lane; i < W; i += 64) { seg[0][q][i] = 0u; seg[1][q][i] = 0u; }
        hl1_seq_wave_sync();
        // (1) the DERATED and DOWN sojourns [ceil(T_j), ceil(T_j+1)) of the window
#pragma unroll
        for (int s = 0; s < 2; ++s) {                        // unrolled: the cursors stay in registers
            if (s >= nslot) break;
            bool more = mine[s];
            while (__any(more)) {
                int fb = 0, fe = 0, fs = 0;                  // fs: the state of the sojourn to fill
                if (more) {
                    const int64_t c = (int64_t)__builtin_ceil(tn[s]);             // the transition takes effect from step c on
                    // c >= w0: the cursor passed every earlier window (but T_1 may underflow to 0, before step 1)
                    const int b = c < w1 ? (c > w0 ? (int)(c - w0) : 0) : W;
                    if (st[s] != 0 && b > since[s]) { fb = since[s]; fe = b; fs = st[s]; }
                    if (c >= w1) { more = false; since[s] = 0; }                  // the cursor waits; its sojourn covers the next window from the first step
                    else {
                        const uint32_t kd = (kind[s] >> (2 * st[s])) & 3u;
                        bool first = kd == 1u;
                        if (kd == 2u) first = hl1_ms_branch_u(chain, lane + 64 * s, ev[s] - 1, seed) < S->first_p[st[s]][lane + 64 * s];
                        // destinations, first-listed / other: UP -> DOWN / DERATED, DERATED -> UP / DOWN, DOWN -> UP / DERATED
                        st[s] = first ? (st[s] == 0 ? 2 : 0) : (st[s] == 1 ? 2 : 1);
                        since[s] = b;
                        const double l = log(hl1_seq_u(chain, lane + 64 * s, ev[s], seed));
                        tn[s] = __dadd_rn(tn[s], __dmul_rn(-hl1_ms_pick(st[s], m0[s], m1[s], m2[s]), l));   // no FMA: the host model rounds the same way
                        ++ev[s];
                    }
                }
                for (uint64_t pend = __ballot(fe > fb); pend; pend &= pend - 1) {
                    const int src = __builtin_ctzll(pend);
                    const int sb = __builtin_amdgcn_readlane(fb, src), se = __builtin_amdgcn_readlane(fe, src), sk = src + 64 * s;
                    uint32_t* const row = seg[__builtin_amdgcn_readlane(fs, src) - 1][sk >> 5];     // fs is 1 or 2 where fe > fb
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
            double cap = 0.0;
            int nder = 0, ndown = 0;
            for (int q = 0; q < nw; ++q) {
                const uint32_t de = valid ? seg[0][q][i] : 0u, dn = valid ? seg[1][q][i] : 0u;
                const int kn = ngen - 32 * q < 32 ? ngen - 32 * q : 32;
                const uint32_t vm = kn < 32 ? (1u << kn) - 1u : ~0u, up = ~dn;
                // ascending units; + 0.0 is exact.  rest (wave-uniform): the units DERATED on some step of the 64-step group.  Without one
                // the sum is relmc_hl1_seq_kernel's, one select per unit; otherwise only the units of `rest` take the second select
                const uint32_t rest = row_or<64>(de) & vm;
                if (rest == 0u) {
                    for (int b = 0; b < kn; ++b) cap += ((up >> b) & 1u) ? S->cap[32 * q + b][0] : 0.0;
                } else {
                    for (int b = 0; b < kn; ++b) {
                        const double* const c = S->cap[32 * q + b];               // (capacity_mw, derated_mw): one scalar load
                        if ((rest >> b) & 1u) cap += ((dn >> b) & 1u) ? 0.0 : ((de >> b) & 1u) ? c[1] : c[0];
                        else cap += ((up >> b) & 1u) ? c[0] : 0.0;
                    }
                }
                nder += __popc(de & vm); ndown += __popc(dn & vm);
            }
            const double ld = load[h];                       // h < H on every lane
            const bool f = valid && cap < ld;
            const double d = f ? ld - cap : 0.0;
            const int fl = __shfl_up((int)f, 1);
            const bool r = f && !(lane == 0 ? prev : fl != 0);
            prev = __shfl((int)f, 63) != 0;
            for (;;) {
                if (valid && y == ycur) { aL += f ? 1u : 0u; aE += d; aF += r ? 1u : 0u; aD += (uint32_t)nder; aN += (uint32_t)ndown; }
                if (!__any(valid && y > ycur)) break;
                hl1_ms_close_year(aL, aE, aF, aD, aN, out0 + (size_t)ycur * 3, out1 + (size_t)ycur * 3);
                ++ycur;
            }
            gh += 64;
            while (gh >= H) { gh -= H; ++gy; }
        }
        hl1_seq_wave_sync();
    }
    hl1_ms_close_year(aL, aE, aF, aD, aN, out0 + (size_t)ycur * 3, out1 + (size_t)ycur * 3);
}
}  // namespace relmc
