// relmc_event_kernels.h — loss events of the HL1 sequential chronology (relmc_hl1_seq_events, contract in include/relmc.h): a loss event
// is a maximal run of consecutive loss steps of a chain; the kernels give every event's start step, duration, energy and peak, the
// per-chain summary records, the duration histogram and the fixed-order reduction of the records.
#pragma once
#include "../../include/relmc.h"
#include "relmc_devfn.h"
#include "relmc_hl1_chrono.h"

namespace relmc {

DEVFI void hl1_event_rec_zero(Hl1EventRec& r)
{
    r.events = r.sum_dur = r.sum_dur2 = r.max_dur = r.censored = 0;
    r.sum_energy = r.sum_energy2 = r.max_energy = r.max_peak = 0.0;
}

// Lane `src`'s value (src wave-uniform) / a value that is the same in every lane, moved into scalar registers: the carry and the chain's
// record are wave-uniform, and held this way they cost no vector register (the kernel keeps relmc_hl1_seq_kernel's occupancy)
DEVFI double hl1_event_lane(double x, int src)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), src), __builtin_amdgcn_readlane(__double2loint(x), src));
}
DEVFI long long hl1_event_lane(long long x, int src)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)x, src), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((unsigned long long)x >> 32), src);
    return (long long)(((unsigned long long)hi << 32) | lo);
}
DEVFI double hl1_event_uniform(double x)
{
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(x)), __builtin_amdgcn_readfirstlane(__double2loint(x)));
}

// a += b (sums first + second: the order is part of the results)
DEVFI void hl1_event_rec_add(Hl1EventRec& a, const Hl1EventRec& b)
{
    a.events += b.events; a.sum_dur += b.sum_dur; a.sum_dur2 += b.sum_dur2; a.censored += b.censored;
    a.max_dur = a.max_dur > b.max_dur ? a.max_dur : b.max_dur;
    a.sum_energy += b.sum_energy; a.sum_energy2 += b.sum_energy2;
    a.max_energy = fmax(a.max_energy, b.max_energy); a.max_peak = fmax(a.max_peak, b.max_peak);
}

// Chain c = blockIdx.x * 4 + wave; the chronology is relmc_hl1_seq_kernel's, word for word (lane l owns units l and l + 64, windows of
// HL1_SEQ_WINDOW steps filled into the wave's LDS masks, one step per lane, no workgroup barrier).  The window loop below is a COPY of
// relmc_hl1_seq_kernel's (relmc_seq_kernels.h), on purpose: the two attempts to share that loop between kernels each cost the
// sequential kernel 1.6-3 %, and this kernel must leave relmc_hl1_seq_kernel's code as it is.
//
// Events of a 64-step group: m = ballot of the lanes' loss flags.  A flagged (segmented) scan over the lanes gives every loss lane the
// deficit sum and maximum of its run from the run's first lane of the group on (6 steps; a lane's run starts behind the highest clear
// bit of m below it).  A lane whose successor has no loss closes its run and owns the event; a run that reaches lane 63 stays open in the
// wave-uniform carry (open, start step, duration, energy, peak), which crosses groups, windows and years and is closed by the first
// later group whose lane 0 has no loss, or by the chain's last step (censored).  Closing lanes are ranked by the ballot, so a chain's
// events are numbered in step order; the chain's record takes them one by one in that order, wave-uniform in scalar registers (a
// per-lane record cost 18 vector registers and with them one wave per SIMD: +3.7 % on the sequential kernel's time instead of -5 %).
// Groups without a loss step and without an open run (nearly all of them) skip all of this.
//   LIST = false: per-chain summary record rec[chain], event count count[chain], duration histogram hist[n_bins] (integer atomics)
//   LIST = true:  event j of the chain goes to events[offset[chain] + j] if that index is below cap; nothing else is written
template <bool LIST>
__global__ void __launch_bounds__(256) relmc_hl1_event_kernel(const Hl1SeqCase* __restrict__ S, const double* __restrict__ load, uint64_t seed,
                                                              uint64_t first_chain, int64_t n_chains, int32_t years, int32_t start, int32_t n_bins,
                                                              unsigned long long* __restrict__ hist, Hl1EventRec* __restrict__ rec,
                                                              long long* __restrict__ count, const long long* __restrict__ offset,
                                                              int64_t chain_base, int64_t cap, relmc_hl1_event* __restrict__ events)
{
    constexpr int W = HL1_SEQ_WINDOW;
    __shared__ uint32_t masks[4][4][W];                     // [wave][mask word][step of the window], bit k & 31 of word k >> 5 = unit k down
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t cl = (int64_t)blockIdx.x * 4 + wv;
    if (cl >= n_chains) return;                              // wave-uniform
    long long off0 = 0;
    if constexpr (LIST) {
        off0 = offset[cl];
        if (off0 >= cap) return;                             // the caller's list is full before this chain (wave-uniform)
    }
    const uint64_t chain = first_chain + (uint64_t)cl;
    const int ngen = S->ngen, H = S->nhours, nw = (ngen + 31) >> 5, nslot = ngen > 64 ? 2 : 1;
    uint32_t (*const seg)[W] = masks[wv];
    const int64_t nsteps = (int64_t)years * H;

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

    Hl1EventRec a;                                           // the chain's record so far (wave-uniform, events = cnt at the end)
    hl1_event_rec_zero(a);
    long long cnt = 0;                                       // events closed so far (wave-uniform)
    bool open = false;                                       // wave-uniform carry: a run that reached the last step before the group
    long long cn0 = 0, cD = 0;
    double cE = 0.0, cP = 0.0;
    // LIST: the event (n0, D, E, P), number j of the chain, stored by the lane that owns it
    auto store = [&](long long n0, long long D, double E, double P, long long j) {
        const long long at = off0 + j;
        if (at < cap) {
            relmc_hl1_event* const e = events + at;
            e->chain = chain_base + cl; e->start_step = n0; e->duration = D; e->energy_mwh = E; e->peak_mw = P;
        }
    };
    // !LIST: one event into the chain's record, by the whole wave (every argument wave-uniform); events in step order
    auto account = [&](long long D, double E, double P, bool censored) {
        a.sum_dur += D; a.sum_dur2 += D * D; a.max_dur = a.max_dur > D ? a.max_dur : D; a.censored += censored ? 1 : 0;
        a.sum_energy = hl1_event_uniform(a.sum_energy + E); a.sum_energy2 = hl1_event_uniform(__builtin_fma(E, E, a.sum_energy2));
        a.max_energy = hl1_event_uniform(fmax(a.max_energy, E)); a.max_peak = hl1_event_uniform(fmax(a.max_peak, P));
    };
    auto count_dur = [&](long long D) {                      // !LIST: the histogram, by the lane that owns the event
        if (hist) atomicAdd(hist + ((D < n_bins ? D : (long long)n_bins) - 1), 1ull);
    };

    int gh = 0;                                              // hour of the year of the current 64-step group's first step
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
                        const int64_t lo = since[s] > w0 ? since[s] : w0, hi = c < w1 ? c : w1;
                        if (hi > lo) { fb = (int)(lo - w0); fe = (int)(hi - w0); }
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
            const int i = g + lane;
            const bool valid = i < wlen;
            int h = gh + lane;
            while (h >= H) h -= H;
            bool f = false;
            double d = 0.0;
            if (valid) {
                double cap_avail = 0.0;
                for (int q = 0; q < nw; ++q) {
                    const uint32_t up = ~seg[q][i];
                    const int kn = ngen - 32 * q < 32 ? ngen - 32 * q : 32;
                    for (int b = 0; b < kn; ++b) cap_avail += ((up >> b) & 1u) ? S->cap[32 * q + b] : 0.0;   // ascending units; + 0.0 is exact
                }
                const double ld = load[h];
                f = cap_avail < ld;
                d = f ? ld - cap_avail : 0.0;
            }
            // (3) the group's events
            const uint64_t m = __ballot(f);                  // lanes past the chain's last step carry no loss
            if (m != 0 || open) {                            // wave-uniform
                const int64_t base = w0 + g;                 // step of lane 0
                if (open && !(m & 1)) {                      // the open run ended with the step before the group
                    if constexpr (LIST) { if (lane == 0) store(cn0, cD, cE, cP, cnt); }
                    else { account(cD, cE, cP, false); if (lane == 0) count_dur(cD); }
                    ++cnt; open = false;
                }
                if (m != 0) {
                    const uint64_t z = ~m & ((1ull << lane) - 1);
                    const int st = z ? 64 - __builtin_clzll(z) : 0;               // first lane of this lane's run in the group
                    double rs = d, rp = d;
#pragma unroll
                    for (int o = 1; o < 64; o <<= 1) {
                        const double vs = __shfl_up(rs, o), vp = __shfl_up(rp, o);
                        if (lane - o >= st) { rs = vs + rs; rp = fmax(vp, rp); }
                    }
                    const bool end63 = base + 63 == nsteps;                       // lane 63 is the chain's last step: its run ends there
                    uint64_t c = m & ~(m >> 1);
                    if (!end63) c &= ~(1ull << 63);
                    const bool cont = open && st == 0;                            // the run came in through the carry
                    const long long n0 = cont ? cn0 : base + st, D = (cont ? cD : 0) + (lane - st + 1);
                    const double E = cont ? cE + rs : rs, P = cont ? fmax(cP, rp) : rp;
                    if constexpr (LIST) {
                        if ((c >> lane) & 1) store(n0, D, E, P, cnt + __popcll(c & ((1ull << lane) - 1)));
                    } else {
                        if ((c >> lane) & 1) count_dur(D);
                        for (uint64_t cc = c; cc; cc &= cc - 1) {                 // ascending lanes = step order
                            const int src = __builtin_ctzll(cc);
                            account(hl1_event_lane(D, src), hl1_event_lane(E, src), hl1_event_lane(P, src), base + src == nsteps);
                        }
                    }
                    cnt += __popcll(c);
                    if ((m >> 63) && !end63) {                                    // lane 63's run goes on into the next group
                        const int st63 = __builtin_amdgcn_readlane(st, 63);
                        const double s63 = hl1_event_lane(rs, 63), p63 = hl1_event_lane(rp, 63);
                        if (open && st63 == 0) { cD += 64; cE = hl1_event_uniform(cE + s63); cP = hl1_event_uniform(fmax(cP, p63)); }
                        else { cn0 = base + st63; cD = 64 - st63; cE = s63; cP = p63; open = true; }
                    } else open = false;
                }
            }
            gh += 64;
            while (gh >= H) gh -= H;
        }
        hl1_seq_wave_sync();
    }
    if constexpr (!LIST) {
        if (lane == 0) { a.events = cnt; rec[cl] = a; count[cl] = cnt; }
    }
}

// offset[i] = count[0] + ... + count[i - 1] for i < n, one workgroup: a contiguous slice per thread, the slices' sums scanned by thread 0
__global__ void __launch_bounds__(256) relmc_hl1_event_scan_kernel(const long long* __restrict__ count, int64_t n, long long* __restrict__ offset)
{
    __shared__ long long tot[256];
    const int tid = threadIdx.x;
    const int64_t per = (n + 255) / 256, lo = tid * per < n ? tid * per : n, hi = lo + per < n ? lo + per : n;
    long long s = 0;
    for (int64_t i = lo; i < hi; ++i) s += count[i];
    tot[tid] = s;
    __syncthreads();
    if (tid == 0) {
        long long run = 0;
        for (int t = 0; t < 256; ++t) { const long long v = tot[t]; tot[t] = run; run += v; }
    }
    __syncthreads();
    s = tot[tid];
    for (int64_t i = lo; i < hi; ++i) { offset[i] = s; s += count[i]; }
}

// Sum of n chain records: grid-stride in a fixed order, then a fixed tree; partial[block] (relmc_hl1_reduce_kernel's pattern)
__global__ void __launch_bounds__(256) relmc_hl1_event_reduce_kernel(const Hl1EventRec* __restrict__ rec, int64_t n, Hl1EventRec* __restrict__ partial)
{
    __shared__ Hl1EventRec red[256];
    const int tid = threadIdx.x;
    Hl1EventRec s;
    hl1_event_rec_zero(s);
    for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < n; i += (int64_t)gridDim.x * 256) hl1_event_rec_add(s, rec[i]);
    red[tid] = s;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off) hl1_event_rec_add(red[tid], red[tid + off]);
        __syncthreads();
    }
    if (tid == 0) partial[blockIdx.x] = red[0];
}
}  // namespace relmc
