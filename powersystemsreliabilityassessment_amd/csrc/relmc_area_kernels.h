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
// COPY = false (relmc_hl1_area_kernel<true>, a step with a tie DOWN): R is the caller's, `tie` is not read.
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
// relmc_hl1_seq_kernel (lane l owns global units l and l + 64; HL1_SEQ_WINDOW steps per window; the whole wave fills one down interval
// at a time).  Per step (one per lane): each area's capacity over its contiguous unit range in ascending order, the margin m_a = cap_a -
// load[a][h] into LDS, the transfer solve only where a margin is negative under INTERCONNECTED, then curtailments c_a = max(-m_a, 0).
// Loss flags are a bit mask per lane (bit a: c_a > 0, bit n: any), so the rising edge is f & ~prev with prev from the neighbouring lane
// (lane 63's mask carried over).  Loss hours and events are wave-uniform counts (ballot + popcount) of the open year; EUE is a lane
// partial per row (the system row sums c_a in area order) closed by a fixed-order butterfly.  Dynamic LDS: margins [n][64], residual
// capacities [n * n][64] (INTERCONNECTED only), then the masks [nw][HL1_SEQ_WINDOW].  Records: rec[row][chain * years + year][3],
// rows `stride` records apart.
// TIES (launched under INTERCONNECTED with one failing tie at least; one more mask row of dynamic LDS): lane t < n_ties carries a third
// cursor slot for tie t (component 128 + t of the draws; mttf = +inf: no cursor, never DOWN), whose down intervals fill the mask row
// seg[nw] (bit t).  A step that needs the transfer solve starts from A->tie when its tie word is 0, else from the UP ties (area_tie_residual).
// Without TIES, TL is not read (the host passes nullptr).
template <bool TIES>
__global__ void __launch_bounds__(64) relmc_hl1_area_kernel(const AreaCase* __restrict__ A, const AreaTies* __restrict__ TL,
                                                            const double* __restrict__ load, uint64_t seed, uint64_t first_chain, int32_t years,
                                                            int32_t start, int32_t policy, int32_t flow, int64_t stride, double* __restrict__ rec)
{
    constexpr int NS = TIES ? 3 : 2;                         // cursor slots per lane: units lane, lane + 64, and tie `lane`
    constexpr int W = HL1_SEQ_WINDOW;
    extern __shared__ double lds[];
    const int lane = threadIdx.x;
    const int64_t cl = blockIdx.x;
    const uint64_t chain = first_chain + (uint64_t)cl;
    const int ngen = A->ngen, H = A->nhours, na = A->n_areas, nw = (ngen + 31) >> 5, nslot = ngen > 64 ? 2 : 1;
    const bool inter = policy == RELMC_HL1_AREA_INTERCONNECTED;
    double* const aE = lds + lane;                           // aE[r * 64]: this lane's EUE partial of row r in the open year ycur
    double* const mg = lds + 64 * (na + 1) + lane;
    double* const R = lds + 64 * (2 * na + 1) + lane;
    uint32_t (*const seg)[W] = reinterpret_cast<uint32_t (*)[W]>(lds + 64 * (2 * na + 1 + (inter ? na * na : 0)));
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

    int cL[AREA_MAX + 1], cF[AREA_MAX + 1];                  // the wave's loss hours / events of the open year, per row (uniform)
#pragma unroll
    for (int r = 0; r <= AREA_MAX; ++r) cL[r] = cF[r] = 0;
    for (int r = 0; r <= na; ++r) aE[r * 64] = 0.0;
    int ycur = 0, gy = 0, gh = 0;
    uint32_t prev = 0u;                                      // loss mask of the step before the group (none before step 1)
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
                    for (int h = sb + lane; h < se; h += 64) row[h] |= bit;
                }
            }
        }
        hl1_seq_wave_sync();
        // (2) one step per lane
        for (int g = 0; g < wlen; g += 64) {
            const int i = g + lane;
            const bool valid = i < wlen;
            int h = gh + lane, y = gy;
            while (h >= H) { h -= H; ++y; }
            uint32_t fw = 0u;
            if (valid) {
                int a = 0, kend = A->lo[1];                  // area a's units end at kend (every area has one unit at least)
                double cap = 0.0;
                bool neg = false;
                for (int q = 0; q < nw; ++q) {
                    const uint32_t up = ~seg[q][i];
                    const int kn = ngen - 32 * q < 32 ? ngen - 32 * q : 32;
                    for (int b = 0; b < kn; ++b) {
                        const int k = 32 * q + b;
                        if (k == kend) {
                            const double m = cap - load[(size_t)a * H + h];
                            mg[a * 64] = m; neg |= m < 0.0;
                            cap = 0.0; ++a; kend = A->lo[a + 1];
                        }
                        cap += ((up >> b) & 1u) ? A->cap[k] : 0.0;                    // ascending units; + 0.0 is exact
                    }
                }
                const double m = cap - load[(size_t)a * H + h];
                mg[a * 64] = m; neg |= m < 0.0;
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
                    if (mg[r * 64] < 0.0) fw |= 1u << r;
                }
                if (fw) fw |= 1u << na;
            }
            const uint32_t fl = (uint32_t)__shfl_up((int)fw, 1);
            const uint32_t rise = fw & ~(lane == 0 ? prev : fl);
            prev = (uint32_t)__shfl((int)fw, 63);
            for (;;) {
                const bool in = valid && y == ycur;
                if (in) {
                    double ds = 0.0;
                    for (int r = 0; r < na; ++r) {
                        const double mr_ = mg[r * 64];
                        const double c = mr_ < 0.0 ? -mr_ : 0.0;
                        aE[r * 64] += c; ds += c;                // the system's deficit: sum of c_a in area order
                    }
                    aE[na * 64] += ds;
                }
#pragma unroll
                for (int r = 0; r <= AREA_MAX; ++r) {                   // a constant trip count: fully unrolled, cL / cF stay in registers
                    if (r <= na) {
                        cL[r] += (int)__popcll(__ballot(in && ((fw >> r) & 1u)));
                        cF[r] += (int)__popcll(__ballot(in && ((rise >> r) & 1u)));
                    }
                }
                if (!__any(valid && y > ycur)) break;
#pragma unroll
                for (int r = 0; r <= AREA_MAX; ++r)
                    if (r <= na) area_close_year(aE[r * 64], cL[r], cF[r], out + (size_t)r * (size_t)stride * 3 + (size_t)ycur * 3);
                ++ycur;
            }
            gh += 64;
            while (gh >= H) { gh -= H; ++gy; }
        }
        hl1_seq_wave_sync();
    }
#pragma unroll
    for (int r = 0; r <= AREA_MAX; ++r)
        if (r <= na) area_close_year(aE[r * 64], cL[r], cF[r], out + (size_t)r * (size_t)stride * 3 + (size_t)ycur * 3);
}
}  // namespace relmc
