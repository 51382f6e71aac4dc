// relmc_seq_event_kernels.h — loss events of the sequential HL2 track (relmc_seq_events, include/relmc.h): count -> offsets -> fill ->
// reduce, behind a relmc_seq_years step, on its per-hour system curtailment curt[years][hpy] and its masks[years][hpy][mw].  The offsets
// are relmc_hl1_event_scan_kernel's (relmc_seq_kernels.h).  Every floating sum is taken in a fixed order; the only atomics are the
// histogram's integer ones.  Launched from relmc_seq.hip alone.
#pragma once
#include "../../include/relmc.h"
#include "relmc_devfn.h"

namespace relmc {

// One 256-hour tile of a year's loss flags: every wavefront's 64 flags as a ballot word in LDS, the run starts of all four words from
// the words themselves (a start = a flag whose hour before has none; `carry` = the flag of the hour before the tile, 0 before hour 0,
// on return the flag of the tile's last hour).  Hours past the year's end come with f = false.  Two barriers; wb is free again on return.
struct SeqEventTile {
    uint64_t starts;        // this wavefront's run starts, bit = lane
    uint32_t wave_off;      // run starts of the tile in the wavefronts before this one
    uint32_t total;         // run starts of the tile
};
DEVFI SeqEventTile seq_event_tile(bool f, int wv, int lane, uint32_t& carry, uint64_t* wb)
{
    const uint64_t b = __ballot(f);
    if (lane == 0) wb[wv] = b;
    __syncthreads();
    SeqEventTile t;
    t.starts = 0; t.wave_off = 0; t.total = 0;
    uint64_t prev = carry;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint64_t w = wb[q], s = w & ~((w << 1) | prev);
        if (q == wv) { t.starts = s; t.wave_off = t.total; }
        t.total += (uint32_t)__popcll(s);
        prev = w >> 63;
    }
    carry = (uint32_t)prev;
    __syncthreads();
    return t;
}

// 1. count[y] = loss events of year y (one workgroup per year)
__global__ void __launch_bounds__(256) relmc_seq_event_count_kernel(const double* __restrict__ curt, int hpy, double threshold, long long* __restrict__ count)
{
    __shared__ uint64_t wb[4];
    const int y = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const double* c = curt + (size_t)y * hpy;
    uint32_t carry = 0;
    long long n = 0;
    for (int h0 = 0; h0 < hpy; h0 += 256) {
        const int h = h0 + tid;
        n += seq_event_tile(h < hpy && c[h] > threshold, wv, lane, carry, wb).total;
    }
    if (tid == 0) count[y] = n;
}

// 3. the events of year y at list[offset[y] ...] in start order (one workgroup per year): the lane that holds a run's start hour walks the
// run to its end -- energy left to right, peak, the OR of the masks -- and stores the record.  Records at or past `cap` are not stored.
__global__ void __launch_bounds__(256) relmc_seq_event_fill_kernel(const double* __restrict__ curt, const uint32_t* __restrict__ masks, int hpy, int mw,
                                                                   double threshold, const long long* __restrict__ offset, long long cap,
                                                                   relmc_seq_event* __restrict__ list)
{
    __shared__ uint64_t wb[4];
    const int y = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const double* c = curt + (size_t)y * hpy;
    const uint32_t* my = masks + (size_t)y * hpy * mw;
    uint32_t carry = 0;
    long long base = offset[y];
    for (int h0 = 0; h0 < hpy; h0 += 256) {
        const int h = h0 + tid;
        const SeqEventTile t = seq_event_tile(h < hpy && c[h] > threshold, wv, lane, carry, wb);
        const long long idx = base + t.wave_off + __popcll(t.starts & ((1ull << lane) - 1ull));
        base += t.total;
        if (!((t.starts >> lane) & 1ull) || idx >= cap) continue;
        relmc_seq_event r;
        const uint32_t* m = my + (size_t)h * mw;
#pragma unroll
        for (int q = 0; q < SEQ_EVENT_MW; ++q) {
            const uint32_t cur = q < mw ? m[q] : 0u, before = q < mw && h > 0 ? m[q - mw] : 0u;
            r.onset[q] = cur & ~before; r.involved[q] = cur;
        }
        double e = 0.0, p = -INFINITY;
        int u = h;
        for (; u < hpy; ++u) {
            const double v = c[u];
            if (!(v > threshold)) break;
            e += v; p = fmax(p, v);
            m = my + (size_t)u * mw;
#pragma unroll
            for (int q = 0; q < SEQ_EVENT_MW; ++q) if (q < mw) r.involved[q] |= m[q];
        }
        r.year = y; r.start_hour = h; r.duration = u - h; r.censored = u == hpy ? 1 : 0;
        r.energy_mwh = e; r.peak_mw = p;
        list[idx] = r;
    }
}

// a += b (sums first + second: the order is part of the results)
DEVFI void seq_event_part_add(SeqEventPart& a, const SeqEventPart& b)
{
    a.events += b.events; a.censored += b.censored; a.load_onset += b.load_onset; a.sum_dur += b.sum_dur; a.sum_dur2 += b.sum_dur2;
    a.max_dur = a.max_dur > b.max_dur ? a.max_dur : b.max_dur;
    a.sum_energy += b.sum_energy; a.sum_energy2 += b.sum_energy2;
    a.max_energy = fmax(a.max_energy, b.max_energy); a.max_peak = fmax(a.max_peak, b.max_peak);
}

// 4a. moments and maxima of the n = min(*total, cap) events the fill stored (total: the scan's last offset, so that no record is read
// that was not written): grid-stride in a fixed order, then a fixed tree; partial[block].  hist (n_bins > 0):
// hist[min(duration, n_bins) - 1] += 1 by integer atomics
__global__ void __launch_bounds__(256) relmc_seq_event_reduce_kernel(const relmc_seq_event* __restrict__ list, const long long* __restrict__ total, long long cap,
                                                                     int n_bins, unsigned long long* __restrict__ hist, SeqEventPart* __restrict__ partial)
{
    __shared__ SeqEventPart red[256];
    const int tid = threadIdx.x;
    const long long n = *total < cap ? *total : cap;
    SeqEventPart s;
    s.events = s.censored = s.load_onset = s.sum_dur = s.sum_dur2 = s.max_dur = 0;
    s.sum_energy = s.sum_energy2 = s.max_energy = s.max_peak = 0.0;
    for (long long i = (long long)blockIdx.x * 256 + tid; i < n; i += (long long)gridDim.x * 256) {
        const relmc_seq_event& r = list[i];
        const long long d = r.duration;
        const double e = r.energy_mwh;
        uint32_t on = 0;
#pragma unroll
        for (int q = 0; q < SEQ_EVENT_MW; ++q) on |= r.onset[q];
        SeqEventPart one;
        one.events = 1; one.censored = r.censored; one.load_onset = on == 0u ? 1 : 0; one.sum_dur = d; one.sum_dur2 = d * d; one.max_dur = d;
        one.sum_energy = e; one.sum_energy2 = e * e; one.max_energy = e; one.max_peak = r.peak_mw;
        seq_event_part_add(s, one);
        if (n_bins > 0) atomicAdd(&hist[(d < n_bins ? d : n_bins) - 1], 1ull);
    }
    red[tid] = s;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off) seq_event_part_add(red[tid], red[tid + off]);
        __syncthreads();
    }
    if (tid == 0) partial[blockIdx.x] = red[0];
}

// 4b. the per-component arrays: lane k walks the list in order for component k (one workgroup of SEQ_NCOMPMAX lanes), so every sum has
// the list's order (n as in the reduction)
__global__ void __launch_bounds__(256) relmc_seq_event_comp_kernel(const relmc_seq_event* __restrict__ list, const long long* __restrict__ total, long long cap,
                                                                   SeqEventComp* __restrict__ out)
{
    const int k = threadIdx.x, w = k >> 5;
    const long long n = *total < cap ? *total : cap;
    const uint32_t bit = 1u << (k & 31);
    long long oc = 0, ic = 0;
    double oe = 0.0, ie = 0.0;
    for (long long i = 0; i < n; ++i) {
        const double e = list[i].energy_mwh;
        if (list[i].onset[w] & bit) { ++oc; oe += e; }
        if (list[i].involved[w] & bit) { ++ic; ie += e; }
    }
    out->onset_events[k] = oc; out->involved_events[k] = ic; out->onset_energy[k] = oe; out->involved_energy[k] = ie;
}
}  // namespace relmc
