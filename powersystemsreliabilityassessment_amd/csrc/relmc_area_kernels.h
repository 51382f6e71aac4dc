// relmc_area_kernels.h — kernel of the HL1 multi-area chronology (GeneratingAdequacy/AdequacyAssessmentII.jl:73-250; contract in
// include/relmc.h): relmc_hl1_seq_kernel's chronology, n area margins and a tie-limited transfer solve per step.
#pragma once
#include "relmc_hl1_chrono.h"

namespace relmc {

// BFS of the transfer solve over this lane's residual capacities R[(u * n + v) * 64]: FIFO queue from s, neighbours in ascending order,
// an area is marked when it is pushed.  t >= 0: the path ends at t (REFERENCE); t < 0: at the first popped area in deficit (MAX_FLOW).
// Parents, queue and marks are 4-bit fields / bits of 32-bit registers (n <= 8).  Returns the sink, or -1 without a path.
DEVFI int area_bfs(const double* __restrict__ mg, const double* __restrict__ R, int n, int s, int t, uint32_t& parent)
{
    uint32_t queue = (uint32_t)s, marked = 1u << s;
    int head = 0, tail = 1;
    parent = 0u;
    while (head < tail) {
        const int u = (int)((queue >> (4 * head)) & 15u);
        ++head;
        if (t >= 0 ? u == t : mg[u * 64] < -1e-4) return u;
        for (int v = 0; v < n; ++v)
            if (!((marked >> v) & 1u) && R[(u * n + v) * 64] > 1e-4) {
                parent = (parent & ~(15u << (4 * v))) | ((uint32_t)u << (4 * v));
                marked |= 1u << v;
                queue |= (uint32_t)v << (4 * tail);
                ++tail;
            }
    }
    return -1;
}

// INTERCONNECTED transfer solve of one lane (:105-167) on its margins mg[a * 64] in LDS, in place; R starts as the topology T.
// REFERENCE: s / t = the lowest area with m > 1e-4 / m < -1e-4, stop when either is missing or s cannot reach t (the reference's break).
// MAX_FLOW: BFS from each source in ascending order to the first deficit it reaches, restart after each augmentation, stop when no source
// reaches a deficit.  Augmentation: f = min(m_s, -m_t, R along the path); m_s -= f, m_t += f, R[p][v] -= f, R[v][p] += f.
// COPY = false (relmc_hl1_area_tie_kernel, a step with a tie DOWN): R is the caller's, `tie` is not read.
template <bool COPY = true>
DEVFI void area_solve(double* __restrict__ mg, double* __restrict__ R, const double* __restrict__ tie, int n, int flow)
{
    if constexpr (COPY)
        for (int e = 0; e < n * n; ++e) R[e * 64] = tie[e];
    for (int it = 0; it < AREA_MAX_AUG; ++it) {
        int s = -1, t = -1;
        uint32_t parent = 0u;
        if (flow == RELMC_HL1_AREA_FLOW_REFERENCE) {
            for (int a = 0; a < n; ++a) {
                const double m = mg[a * 64];
                if (s < 0 && m > 1e-4) s = a;
                if (t < 0 && m < -1e-4) t = a;
            }
            if (s < 0 || t < 0 || area_bfs(mg, R, n, s, t, parent) < 0) return;
        } else {
            for (int a = 0; a < n && t < 0; ++a)
                if (mg[a * 64] > 1e-4) { s = a; t = area_bfs(mg, R, n, a, -1, parent); }
            if (t < 0) return;
        }
        double f = mg[s * 64], d = -mg[t * 64];
        f = d < f ? d : f;
        for (int v = t; v != s;) {
            const int p = (int)((parent >> (4 * v)) & 15u);
            const double r = R[(p * n + v) * 64];
            f = r < f ? r : f;
            v = p;
        }
        mg[s * 64] -= f;
        mg[t * 64] += f;
        for (int v = t; v != s;) {
            const int p = (int)((parent >> (4 * v)) & 15u);
            R[(p * n + v) * 64] -= f;
            R[(v * n + p) * 64] += f;
            v = p;
        }
    }
}

// R of a step in which the ties of the mask `down` (bit t: tie t) are DOWN: from 0.0, the UP ties' capacities in ascending tie order
DEVFI void area_tie_residual(double* __restrict__ R, const AreaTies* __restrict__ TL, int n, uint32_t down)
{
    for (int e = 0; e < n * n; ++e) R[e * 64] = 0.0;
    const int nt = TL->n_ties;
    for (int t = 0; t < nt; ++t)
        if (!((down >> t) & 1u)) {
            const int i = TL->from[t], j = TL->to[t];
            R[(i * n + j) * 64] += TL->cap[t];
            R[(j * n + i) * 64] += TL->cap[t];
        }
}

// Row r (areas 0..n-1, the system n) of the wave's open year: fixed-order butterfly of the EUE partials, lane 0 stores (loss hours, EUE,
// loss events) to rec[r][record][3]; the row restarts at zero
DEVFI void area_close_year(double& e_lds, int& l, int& f, double* __restrict__ out)
{
    double e = e_lds;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) e += __shfl_xor(e, off);
    if (threadIdx.x == 0) { out[0] = (double)l; out[1] = e; out[2] = (double)f; }
    e_lds = 0.0; l = f = 0;
}

// Chain c = first_chain + blockIdx.x: one wavefront per workgroup, one chain per wavefront.  The cursors and the window masks are those of
// relmc_hl1_seq_kernel (lane l owns global units l and l + 64; HL1_SEQ_WINDOW steps per window; the whole wave fills one down interval at a
// time).  Per step (one per lane): each area's capacity over its contiguous unit range in ascending order, the margin m_a = cap_a -
// load[a][h] into LDS, the transfer solve only where a margin is negative under INTERCONNECTED, then curtailments c_a = max(-m_a, 0).
// Loss flags are a bit mask per lane (bit a: c_a > 0, bit n: any), so the rising edge is f & ~prev with prev from the neighbouring lane
// (lane 63's mask carried over).  Loss hours and events are wave-uniform counts (ballot + popcount) of the open year; EUE is a lane
// partial per row (the system row sums c_a in area order) closed by a fixed-order butterfly.  Dynamic LDS: margins [n][64], residual
// capacities [n * n][64] (INTERCONNECTED only), then the masks [nw][HL1_SEQ_WINDOW].  Records: rec[row][chain * years + year][3],
// rows `stride` records apart.
// TIES (relmc_hl1_area_tie_kernel, INTERCONNECTED only): lane t < n_ties carries a third cursor for tie t (component 128 + t of the draws;
// mttf = +inf: no cursor, never DOWN), whose down intervals fill one more mask row seg[nw] (bit t).  A step that needs the transfer solve
// starts from A->tie when its tie word is 0, else from the UP ties (area_tie_residual).  Without TIES the body is the kernel it was.
//   The body is relmc_area_chain_body.h.

__global__ void __launch_bounds__(64) relmc_hl1_area_kernel(const AreaCase* __restrict__ A, const double* __restrict__ load, uint64_t seed,
                                                            uint64_t first_chain, int32_t years, int32_t start, int32_t policy, int32_t flow,
                                                            int64_t stride, double* __restrict__ rec)
#define RELMC_AREA_TIES 0
#include "relmc_area_chain_body.h"
#undef RELMC_AREA_TIES

// The chronology with tie outages (TL: the ties one by one).  Launched under INTERCONNECTED with one failing tie at least; dynamic LDS as
// above plus one mask row.
__global__ void __launch_bounds__(64) relmc_hl1_area_tie_kernel(const AreaCase* __restrict__ A, const AreaTies* __restrict__ TL,
                                                                const double* __restrict__ load, uint64_t seed, uint64_t first_chain,
                                                                int32_t years, int32_t start, int32_t policy, int32_t flow, int64_t stride,
                                                                double* __restrict__ rec)
#define RELMC_AREA_TIES 1
#include "relmc_area_chain_body.h"
#undef RELMC_AREA_TIES
}  // namespace relmc
