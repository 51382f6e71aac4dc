// relmc_storage_kernels.h — energy storage with a state of charge on the HL1 sequential chronology (relmc_hl1_seq_storage, contract in
// include/relmc.h): one walk of a chain's fleet history against the load L(h) = scale * load[h] + shift, with up to
// RELMC_HL1_MAX_STORAGE storages that discharge into a shortfall and charge from surplus generation.  An extension beyond the reference
// (its only energy-limited resource, the ELU of the planning model, drains and never recharges, on an hourly-sampling Monte Carlo).
// The storage step, the wave-uniform bits and the year close are relmc_hl1_storage_devfn.h's, shared with the weather-year kernels.
#pragma once
#include "relmc_hl1_chrono.h"
#include "relmc_hl1_storage_devfn.h"

namespace relmc {

// The storages and the load level, passed BY VALUE as a kernel argument (as Hl1SweepArgs): every read of a storage's data is a scalar
// load from the kernel argument segment.  st[n_storage ..] is zero and never read.
struct Hl1StorageArgs {
    relmc_hl1_storage st[RELMC_HL1_MAX_STORAGE];
    double scale, shift;
    int32_t n_storage, pad;
};

// Chain c = blockIdx.x * 4 + wave; the chronology is relmc_hl1_seq_kernel's, word for word (lane l owns units l and l + 64, windows of
// HL1_SEQ_WINDOW steps filled into the wave's LDS masks, one step per lane, no workgroup barrier).  The window loop below is a COPY of
// relmc_hl1_seq_kernel's (relmc_seq_kernels.h), on purpose, as relmc_hl1_sweep_kernel's is: sharing that loop between kernels cost the
// sequential kernel 1.6-3 % twice.
//
// Storage i's state of charge lives in lane i of one register for the whole chain; what each storage can still do is kept beside it as
// wave-uniform bits (hl1_storage_bits).  Per 64-step group:
//   parallel   each lane forms cap and L of its step, the flags short (cap < L) and long (cap > L), and m = L - cap or cap - L
//   quiet      no lane is short and every storage is settled (full, or unable to charge): the group changes no state and has no loss;
//              nothing further is done (nearly every group).  A skipped group would add only + 0.0 to the year partials, so the
//              years are closed when a later year shows up in a group that is not quiet, or at the end of the chain
//   serial     the steps on which a storage can act are visited in step order by a wave-uniform loop: the short steps while some
//              storage can discharge (s > 0 and discharge_mw > 0), the long steps while some storage is not settled (both read off
//              the bits).  A step left out is one on which the contract's loop changes nothing: avail or y is 0 for every storage.
//              m of the step is read from its lane, the storages are taken in ascending order, and what is left of the need and
//              the step's sum of x (or of y) go back to the lane
//   year       loss flag, rising edge (the neighbouring lane's flag, lane 63's carried over) and the lane partials of the open year as in
//              relmc_hl1_seq_kernel: the EUE of a year is summed in its order (the counts are kept as integers, exact in any order)
// Records: year_out[row][chain of the launch][year][3], row 0 = (lole, eue, lolf), row 1 = (served_hours, discharged_mwh, charged_mwh).
__global__ void __launch_bounds__(256) relmc_hl1_storage_kernel(const Hl1SeqCase* __restrict__ S, const double* __restrict__ load, uint64_t seed,
                                                                uint64_t first_chain, int64_t n_chains, int32_t years, int32_t start,
                                                                const Hl1StorageArgs A, double* __restrict__ year_out)
{
    constexpr int W = HL1_SEQ_WINDOW;
    constexpr int NS = RELMC_HL1_MAX_STORAGE;
    __shared__ uint32_t masks[4][4][W];                     // [wave][mask word][step of the window], bit k & 31 of word k >> 5 = unit k down
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t cl = (int64_t)blockIdx.x * 4 + wv;
    if (cl >= n_chains) return;                              // wave-uniform
    const uint64_t chain = first_chain + (uint64_t)cl;
    const int ngen = S->ngen, H = S->nhours, nw = (ngen + 31) >> 5, nslot = ngen > 64 ? 2 : 1;
    const int ns = A.n_storage < NS ? A.n_storage : NS;
    uint32_t (*const seg)[W] = masks[wv];
    const int64_t nsteps = (int64_t)years * H;
    double* const out0 = year_out + (size_t)cl * (size_t)years * 3;
    double* const out1 = out0 + (size_t)n_chains * (size_t)years * 3;

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

    double soc = 0.0;                                        // storage i's state of charge (MWh) in lane i
    uint32_t bits = 0u;                                      // hl1_storage_bits of every storage (wave-uniform)
    hl1_storage_each([&](auto ic) {
        constexpr int i = decltype(ic)::value;
        if (i < ns) { soc = lane == i ? A.st[i].soc0_mwh : soc; bits |= hl1_storage_bits(A.st[i], A.st[i].soc0_mwh, i); }
    });
    Hl1StoragePartials a = {0u, 0u, 0u, 0.0, 0.0, 0.0};     // this lane's partials of the open year ycur
    int ycur = 0, gy = 0, gh = 0;                            // gy / gh: chain year and hour of the current 64-step group's first step
    bool prev = false;                                       // loss flag of the step before the group (none before step 1)
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
                        const int64_t a0 = since[s] > w0 ? since[s] : w0, b = c < w1 ? c : w1;
                        if (b > a0) { fb = (int)(a0 - w0); fe = (int)(b - w0); }
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
            bool sh = false, lg = false;                     // short: cap < L, long: cap > L
            double m = 0.0;                                  // the step's need (short) or surplus (long)
            if (valid) {
                double cap = 0.0;
                for (int q = 0; q < nw; ++q) {
                    const uint32_t up = ~seg[q][i];
                    const int kn = ngen - 32 * q < 32 ? ngen - 32 * q : 32;
                    for (int b = 0; b < kn; ++b) cap += ((up >> b) & 1u) ? S->cap[32 * q + b] : 0.0;   // ascending units; + 0.0 is exact
                }
                const double L = hl1_storage_load(A.scale, load[h], A.shift);
                sh = cap < L; lg = cap > L;
                m = sh ? L - cap : lg ? cap - L : 0.0;
            }
            const uint64_t ms = __builtin_amdgcn_ballot_w64(sh), ml = __builtin_amdgcn_ballot_w64(lg);
            if (ms != 0 || (bits >> 8) != 0u) {              // wave-uniform; a quiet group (no short step, every storage settled) does nothing
                double xy = 0.0;                             // the sum of x (short step) or of y (long step) of the lane's step
                int z = 0;
                __asm__ volatile("" : "+s"(z));
                uint64_t rest = ~0ull;                       // the steps after the one just visited
                for (;;) {
                    const uint64_t todo = (((bits & 0xffu) ? ms : 0ull) | ((bits >> 8) ? ml : 0ull)) & rest;
                    if (todo == 0) break;
                    const int j = __builtin_ctzll(todo);
                    rest = j == 63 ? 0ull : ~0ull << (j + 1);
                    const double mj = hl1_storage_readlane(m, j);
                    if ((ms >> j) & 1ull) {
                        double need = mj, x = 0.0;
                        hl1_storage_discharge(A, ns, z, lane, soc, bits, need, x);
                        if (lane == j) { m = need; xy = x; }     // m: what is left of the need
                    } else {
                        double yj = 0.0;
                        hl1_storage_charge(A, ns, z, lane, soc, bits, mj, yj);
                        if (lane == j) xy = yj;
                    }
                }
                const bool f = sh && m > 0.0;                // a loss step: need is left after the storages (m: the deficit)
                const int fl = __shfl_up((int)f, 1);
                const bool r = f && !(lane == 0 ? prev : fl != 0);
                prev = __shfl((int)f, 63) != 0;
                for (;;) {
                    if (valid && y == ycur) {
                        a.lole += f ? 1u : 0u; a.lolf += r ? 1u : 0u; a.served += (sh && !f) ? 1u : 0u;
                        a.eue += f ? m : 0.0; a.dis += sh ? xy : 0.0; a.chg += sh ? 0.0 : xy;
                    }
                    if (!__any(valid && y > ycur)) break;
                    hl1_storage_close_year(a, out0 + (size_t)ycur * 3, out1 + (size_t)ycur * 3);
                    ++ycur;
                }
            } else prev = false;
            gh += 64;
            while (gh >= H) { gh -= H; ++gy; }
        }
        hl1_seq_wave_sync();
    }
    for (; ycur < years; ++ycur) hl1_storage_close_year(a, out0 + (size_t)ycur * 3, out1 + (size_t)ycur * 3);
}
}  // namespace relmc
