// relmc_area_kernels.h — kernel of the HL1 multi-area chronology (GeneratingAdequacy/AdequacyAssessmentII.jl:73-250; contract in
// include/relmc.h): relmc_hl1_seq_kernel's chronology, n area margins and a tie-limited transfer solve per step; with the argument of
// relmc_area_variable_devfn.h, weather-year resources and storages in the areas (relmc_hl1_area_var).
#pragma once
#include "relmc_hl1_chrono.h"
#include "relmc_area_variable_devfn.h"

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

// R of a step in which the ties of the mask `down` (bit t: tie t) are DOWN: from 0.0, the UP ties' capacities cap[t] in ascending tie
// order (TL->cap, or those of a level of relmc_hl1_area_sweep)
DEVFI void area_tie_residual(double* __restrict__ R, const AreaTies* __restrict__ TL, const double* __restrict__ cap, int n, uint32_t down)
{
    for (int e = 0; e < n * n; ++e) R[e * 64] = 0.0;
    const int nt = TL->n_ties;
    for (int t = 0; t < nt; ++t)
        if (!((down >> t) & 1u)) {
            const int i = TL->from[t], j = TL->to[t];
            R[(i * n + j) * 64] += cap[t];
            R[(j * n + i) * 64] += cap[t];
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
// at a time).  One template for relmc_hl1_area (VAR empty) and relmc_hl1_area_var (VAR = AreaVarArgs, one more by-value argument ahead
// of rec; a parameter pack so that the kernels without it keep their argument segment): the cursor slots and the window fill are one
// text, the step stage and the year close are each model's own under `if constexpr (VARK)`.  All four instantiations have the
// instructions they had as two templates; that needs `mg`, `R` and `seg` in each model's own words below, and a `close`
// that captures nothing where it is not used.
// Without weather years, per step (one per lane): each area's capacity over its contiguous unit range in ascending order, the margin m_a =
// cap_a - load[a][h] into LDS, the transfer solve only where a margin is negative under INTERCONNECTED, then curtailments c_a = max(-m_a, 0).
// Loss flags are a bit mask per lane (bit a: c_a > 0, bit n: any), so the rising edge is f & ~prev with prev from the neighbouring lane
// (lane 63's mask carried over).  Loss hours and events are wave-uniform counts (ballot + popcount) of the open year; EUE is a lane
// partial per row (the system row sums c_a in area order) closed by a fixed-order butterfly.  Dynamic LDS: margins [n][64], residual
// capacities [n * n][64] (INTERCONNECTED only), then the masks [nw][HL1_SEQ_WINDOW].  Records: rec[row][chain * years + year][3],
// rows `stride` records apart.
// TIES (launched under INTERCONNECTED with one failing tie at least; one more mask row of dynamic LDS): lane t < n_ties carries a third
// cursor slot for tie t (component 128 + t of the draws; mttf = +inf: no cursor, never DOWN), whose down intervals fill the mask row
// seg[nw] (bit t).  A step that needs the transfer solve starts from A->tie when its tie word is 0, else from the UP ties (area_tie_residual).
// Without TIES, TL is not read (the host passes nullptr).
// With weather years, per 64-step group:
//   parallel stage, one step per lane
//     weather    the lane keeps (yw, w * H) of its chain year and works the pick out only when the year changes (as the weather track)
//     loads      L_a = lscale[a] * base_a(w, h) + lshift[a] of every area into the margin slots, and the first two resource outputs, are
//                read AHEAD of the capacity sum, whose work hides their latency; 32-bit library indices
//     capacity   the units walk with the area close-outs; a close-out adds the area's resources r ascending and leaves m_a = cap_a - L_a
//     transfers  the solve only on lanes with a negative margin under INTERCONNECTED: the contract puts the ties before the storages, so
//                the solve needs no state of charge and stays in this stage
//   quiet test   no lane has a margin < 0 left and every storage is settled: the group is skipped on a wave-uniform branch; years are
//                closed lazily, their sums bitwise what they would be (+ 0.0)
//   serial stage in step order, only the steps on which a storage can act (an area short that holds a storage able to discharge, or long
//                with one not settled): area_var_storage_step.  States of charge in the lanes of one register pair.
//   then the flags, rising edges, wave-uniform counts and year closes as above, for both record rows.
// Dynamic LDS: area_var_lds_rows rows of 64 doubles, then the masks [nw (+ 1 with TIES)][HL1_SEQ_WINDOW].
// Records: rec[slice][chain of the launch * years + year][3], slices `stride` records apart: slice r = row r's (lole, eue, lolf),
// slice n_areas + 1 + r = row r's (served_hours, discharged_mwh, charged_mwh); row n_areas is the system.
template <bool TIES, class... VAR>
__global__ void __launch_bounds__(64) relmc_hl1_area_kernel(const AreaCase* __restrict__ A, const AreaTies* __restrict__ TL,
                                                            const double* __restrict__ load, uint64_t seed, uint64_t first_chain,
                                                            int32_t years, int32_t start, int32_t policy, int32_t flow, int64_t stride,
                                                            const VAR... Vp, double* __restrict__ rec)
{
    constexpr bool VARK = sizeof...(VAR) != 0;
    constexpr int NS = TIES ? 3 : 2;                         // cursor slots per lane: units lane, lane + 64, and tie `lane`
    constexpr int W = HL1_SEQ_WINDOW;
    extern __shared__ double lds[];
    const int lane = threadIdx.x;
    const int64_t cl = blockIdx.x;
    const uint64_t chain = first_chain + (uint64_t)cl;
    const int ngen = A->ngen, H = A->nhours, na = A->n_areas, nw = (ngen + 31) >> 5, nslot = ngen > 64 ? 2 : 1;
    const bool inter = policy == RELMC_HL1_AREA_INTERCONNECTED;
    const int ns = area_var_ns(Vp...);
    const int nres = area_var_nres(Vp...);
    const bool stor = ns > 0;
    const int rows0 = na + 1, rowsS = stor ? 2 * (na + 1) + na : 0;
    double* const aE = lds + lane;                           // aE[r * 64]: this lane's EUE partial of row r in the open year ycur
    double* const aD = lds + 64 * rows0 + lane;              // stor only: MWh discharged / charged partials of row r, and
    double* const aC = aD + 64 * (na + 1);
    double* const xyw = lds + 64 * (rows0 + 2 * (na + 1));   //   xyw[a * 64 + j]: the x or y sum of area a in step j of the group
    double* const mgw = lds + 64 * (rows0 + rowsS);          // mgw[a * 64 + j]: the margin of area a in step j
    double* const mg = VARK ? mgw + lane : lds + 64 * (na + 1) + lane;
    double* const R = VARK ? mgw + 64 * na + lane : lds + 64 * (2 * na + 1) + lane;
    uint32_t (*const seg)[W] = reinterpret_cast<uint32_t (*)[W]>(lds + 64 * (VARK ? area_var_lds_rows(na, inter, stor) : 2 * na + 1 + (inter ? na * na : 0)));
    const double* __restrict__ const lcurve = area_var_wload(Vp...) ? area_var_wload(Vp...) : load;
    const uint32_t lmask = area_var_wload(Vp...) ? ~0u : 0u;
    const double* __restrict__ const rout = area_var_out(Vp...);
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

    double soc = 0.0;                                        // storage i's state of charge (MWh) in lane i
    uint32_t bits = 0u;                                      // hl1_storage_bits of every storage (wave-uniform)
    if constexpr (VARK) {
        const AreaVarArgs& V = area_var_args(Vp...);
        hl1_storage_each([&](auto ic) {
            constexpr int i = decltype(ic)::value;
            if (i < ns) { soc = lane == i ? V.st[i].soc0_mwh : soc; bits |= hl1_storage_bits(V.st[i], V.st[i].soc0_mwh, i); }
        });
    }
    int cL[AREA_MAX + 1], cF[AREA_MAX + 1], cS[AREA_MAX + 1];   // the wave's loss hours / events / served hours of the open year, per row (uniform)
#pragma unroll
    for (int r = 0; r <= AREA_MAX; ++r) cL[r] = cF[r] = cS[r] = 0;
    for (int r = 0; r <= na; ++r) {
        aE[r * 64] = 0.0;
        if (stor) { aD[r * 64] = 0.0; aC[r * 64] = 0.0; }
    }
    int ycur = 0, gy = 0, gh = 0;
    int yw = -1;                                             // this lane's cached chain year, and
    uint32_t wb = 0u;                                        // w * H of its weather year w
    uint32_t prev = 0u;                                      // loss mask of the step before the group (none before step 1)
    const auto close = [&](int r) {
        if constexpr (VARK)
            area_var_close_year(aE[r * 64], stor ? aD + r * 64 : nullptr, stor ? aC + r * 64 : nullptr, cL[r], cF[r], cS[r],
                                out + (size_t)r * (size_t)stride * 3 + (size_t)ycur * 3,
                                out + (size_t)(na + 1 + r) * (size_t)stride * 3 + (size_t)ycur * 3);
    };
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
            if constexpr (VARK) {
                const AreaVarArgs& V = area_var_args(Vp...);
                uint32_t sw = 0u, lw = 0u;                       // bit a: area a is short (m'_a < 0) / long (m'_a > 0) after the transfers
                if (valid) {                                     // y < years, h < H: every read below is inside its table
                    if (y != yw) { yw = y; wb = (uint32_t)hl1_var_weather(seed, chain, y, years, V.n_weather, V.pick) * (uint32_t)H; }
                    const uint32_t oi = wb * (uint32_t)nres + (uint32_t)h;            // out[(w * n_res + r) * H + h], r = 0
                    double o0 = 0.0, o1 = 0.0;
                    if (nres > 0) o0 = rout[oi];                                      // wave-uniform tests
                    if (nres > 1) o1 = rout[oi + (uint32_t)H];
                    {
                        uint32_t li = ((wb * (uint32_t)na) & lmask) + (uint32_t)h;    // lcurve[(w * na + a) * H + h], a = 0
                        for (int a = 0; a < na; ++a, li += (uint32_t)H) mg[a * 64] = hl1_storage_load(V.lscale[a], lcurve[li], V.lshift[a]);
                    }
                    // area a's close-out: its resources r ascending, then m_a = cap_a - L_a in L_a's slot
                    const auto close_out = [&](int a, double cap) -> bool {
#pragma unroll
                        for (int r = 0; r < RELMC_HL1_VAR_MAX_RESOURCES; ++r)
                            if (r < nres && V.rarea[r] == a) {                        // wave-uniform
                                const double o = r == 0 ? o0 : r == 1 ? o1 : rout[oi + (uint32_t)r * (uint32_t)H];
                                cap = hl1_var_add(cap, V.rscale[r], o);
                            }
                        const double m = cap - mg[a * 64];
                        mg[a * 64] = m;
                        return m < 0.0;
                    };
                    int a = 0, kend = A->lo[1];                  // area a's units end at kend (every area has one unit at least)
                    double cap = 0.0;
                    bool neg = false;
                    for (int q = 0; q < nw; ++q) {
                        const uint32_t up = ~seg[q][i];
                        const int kn = ngen - 32 * q < 32 ? ngen - 32 * q : 32;
                        for (int b = 0; b < kn; ++b) {
                            const int k = 32 * q + b;
                            if (k == kend) {
                                neg |= close_out(a, cap);
                                cap = 0.0; ++a; kend = A->lo[a + 1];
                            }
                            cap += ((up >> b) & 1u) ? A->cap[k] : 0.0;                    // ascending units; + 0.0 is exact
                        }
                    }
                    neg |= close_out(a, cap);
                    if constexpr (TIES) {
                        if (inter && neg) {
                            const uint32_t tdown = seg[nw][i];
                            if (tdown) { area_tie_residual(R, TL, TL->cap, na, tdown); area_solve<false>(mg, R, nullptr, na, flow); }
                            else area_solve(mg, R, A->tie, na, flow);
                        }
                    } else if (inter && neg) area_solve(mg, R, A->tie, na, flow);
#pragma unroll
                    for (int r = 0; r < AREA_MAX; ++r) {
                        if (r >= na) break;
                        const double m = mg[r * 64];
                        if (m < 0.0) sw |= 1u << r;
                        if (stor && m > 0.0) lw |= 1u << r;
                    }
                }
                if (__ballot(sw != 0u) != 0ull || (bits >> 8) != 0u) {               // wave-uniform; a quiet group does nothing
                    uint32_t fw = sw;                            // bit a: a deficit is left in area a after the storages; bit na: in any
                    if (stor) {
                        for (int r = 0; r < na; ++r) xyw[r * 64 + lane] = 0.0;
                        hl1_seq_wave_sync();                     // the lanes' margins and zeros, before the wave reads them step by step
                        int z = 0;
                        __asm__ volatile("" : "+s"(z));
                        uint64_t rest = ~0ull;                   // the steps after the one just visited
                        for (;;) {
                            const uint32_t can = area_var_can(V, ns, bits);
                            const uint64_t todo = __ballot(valid && ((sw & can) | (lw & (can >> 16))) != 0u) & rest;
                            if (todo == 0) break;
                            const int j = __builtin_ctzll(todo);
                            rest = j == 63 ? 0ull : ~0ull << (j + 1);
                            area_var_storage_step(V, ns, z, lane, j, mgw, xyw, soc, bits);
                        }
                        hl1_seq_wave_sync();
                        fw = 0u;
                        if (valid) {
#pragma unroll
                            for (int r = 0; r < AREA_MAX; ++r) {
                                if (r >= na) break;
                                if (((sw >> r) & 1u) && mg[r * 64] < 0.0) fw |= 1u << r;
                            }
                        }
                    }
                    uint32_t sv = sw & ~fw;                      // bit a: area a was short after the transfers and is served; bit na: the system
                    if (sw != 0u && fw == 0u) sv |= 1u << na;
                    if (fw) fw |= 1u << na;
                    const uint32_t fl = (uint32_t)__shfl_up((int)fw, 1);
                    const uint32_t rise = fw & ~(lane == 0 ? prev : fl);
                    prev = (uint32_t)__shfl((int)fw, 63);
                    for (;;) {
                        const bool in = valid && y == ycur;
                        if (in) {
                            double ds = 0.0, dd = 0.0, dc = 0.0;
                            for (int r = 0; r < na; ++r) {
                                const double mr_ = mg[r * 64];
                                const double c = ((fw >> r) & 1u) ? -mr_ : 0.0;
                                aE[r * 64] += c; ds += c;                // the system's deficit: sum of c_a in area order
                                if (stor) {
                                    const double xy = xyw[r * 64 + lane];
                                    const bool shr = (sw >> r) & 1u;
                                    const double xd = shr ? xy : 0.0, xc = shr ? 0.0 : xy;
                                    aD[r * 64] += xd; aC[r * 64] += xc; dd += xd; dc += xc;
                                }
                            }
                            aE[na * 64] += ds;
                            if (stor) { aD[na * 64] += dd; aC[na * 64] += dc; }
                        }
#pragma unroll
                        for (int r = 0; r <= AREA_MAX; ++r) {                   // a constant trip count: fully unrolled, the counts stay in registers
                            if (r <= na) {
                                cL[r] += (int)__popcll(__ballot(in && ((fw >> r) & 1u)));
                                cF[r] += (int)__popcll(__ballot(in && ((rise >> r) & 1u)));
                                if (stor) cS[r] += (int)__popcll(__ballot(in && ((sv >> r) & 1u)));
                            }
                        }
                        if (!__any(valid && y > ycur)) break;
#pragma unroll
                        for (int r = 0; r <= AREA_MAX; ++r)
                            if (r <= na) close(r);
                        ++ycur;
                    }
                } else prev = 0u;
            } else {
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
                            if (tdown) { area_tie_residual(R, TL, TL->cap, na, tdown); area_solve<false>(mg, R, nullptr, na, flow); }
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
            }
            gh += 64;
            while (gh >= H) { gh -= H; ++gy; }
        }
        hl1_seq_wave_sync();
    }
    if constexpr (VARK) {
        for (; ycur < years; ++ycur) {
#pragma unroll
            for (int r = 0; r <= AREA_MAX; ++r)
                if (r <= na) close(r);
        }
    } else {
#pragma unroll
        for (int r = 0; r <= AREA_MAX; ++r)
            if (r <= na) area_close_year(aE[r * 64], cL[r], cF[r], out + (size_t)r * (size_t)stride * 3 + (size_t)ycur * 3);
    }
}
}  // namespace relmc
