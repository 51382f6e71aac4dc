// relmc_variable_kernels.h — weather-year wind and solar resources on the HL1 sequential chronology, with storage (relmc_hl1_var_seq,
// contract in include/relmc.h): one walk of a chain's fleet history in which every chain year draws a weather year w of the library of
// relmc_hl1_var_load; the step's capacity is the fleet's plus resource_scale[r] * output[w][r][h], its load scale * base(w, h) + shift, and
// the storages of relmc_hl1_seq_storage act on the two.  An extension beyond the reference, whose generation is all dispatchable.
// The weather pick, the storage step and the year close are relmc_hl1_storage_devfn.h's, one copy for every kernel that uses them.
#pragma once
#include "relmc_hl1_chrono.h"
#include "relmc_hl1_storage_devfn.h"

namespace relmc {

// The storages, the load level, the resource scales and the weather library, passed BY VALUE as a kernel argument (as Hl1StorageArgs):
// every read of them is a scalar load from the kernel argument segment.  st[n_storage ..] and rscale[n_res ..] are zero and never read.
struct Hl1VarArgs {
    relmc_hl1_storage st[RELMC_HL1_MAX_STORAGE];
    double rscale[RELMC_HL1_VAR_MAX_RESOURCES];
    double scale, shift;
    const double* out;                   // [n_weather][n_res][H], fewer than 2^31 values (relmc_hl1_var_load): the kernel indexes it in 32 bits
    const double* wload;                 // [n_weather][H], or nullptr: the load curve of relmc_hl1_seq_load
    int32_t n_storage, n_res, n_weather, pick;
};

// Chain c = blockIdx.x * 4 + wave.  The window loop and the group stages are a COPY of relmc_hl1_storage_kernel's (relmc_storage_kernels.h,
// which says what the stages do), on purpose, as that kernel's is of relmc_hl1_seq_kernel's: sharing the loop between kernels cost the
// sequential kernel 1.6-3 % twice.  What is new is in the parallel stage, one step per lane:
//   weather    a 64-step group may span several years when H < 64, so the weather year belongs to the lane's chain year y.  Each lane
//              keeps (yw, w * H) and works the pick out only when its y changes: once per lane and year, never per step
//   load       base(w, h) from the library's [w][h] curves or the sequential model's [h]: pointer and row mask chosen once per kernel
//   resources  cap = cap + rscale[r] * out[(w * n_res + r) * H + h] for r ascending, lanes on consecutive h (a lane past a year edge reads
//              another row), in 32-bit indices; the scales are scalar loads from the argument segment under wave-uniform tests; the first two
//              outputs and the load are read ahead of the capacity sum, the others in pairs
// The quiet-group test, the serial stage with its wave-uniform bits and the fixed-order year close are the storage kernel's.
// Records: year_out[row][chain of the launch][year][3], row 0 = (lole, eue, lolf), row 1 = (served_hours, discharged_mwh, charged_mwh).
__global__ void __launch_bounds__(256) relmc_hl1_var_kernel(const Hl1SeqCase* __restrict__ S, const double* __restrict__ load, uint64_t seed,
                                                            uint64_t first_chain, int64_t n_chains, int32_t years, int32_t start,
                                                            const Hl1VarArgs A, double* __restrict__ year_out)
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
    const int nres = A.n_res < RELMC_HL1_VAR_MAX_RESOURCES ? A.n_res : RELMC_HL1_VAR_MAX_RESOURCES;
    const double* __restrict__ const lcurve = A.wload ? A.wload : load;       // base(w, h) = lcurve[(w * H & lmask) + h]
    const uint32_t lmask = A.wload ? ~0u : 0u;
    const double* __restrict__ const rout = A.out;
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
    Hl1StoragePartials a = {0u, 0u, 0u, 0.0, 0.0, 0.0};         // this lane's partials of the open year ycur
    int ycur = 0, gy = 0, gh = 0;                            // gy / gh: chain year and hour of the current 64-step group's first step
    int yw = -1;                                             // this lane's cached chain year, and
    uint32_t wb = 0u;                                        // w * H of its weather year w (relmc_hl1_var_load: n_weather * n_res * H < 2^31)
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
            if (valid) {                                     // y < years, h < H: every read below is inside its table
                if (y != yw) { yw = y; wb = (uint32_t)hl1_var_weather(seed, chain, y, years, A.n_weather, A.pick) * (uint32_t)H; }
                // the step's load and its first two outputs are read BEFORE the capacity sum, whose work hides their latency
                const double ld = lcurve[(wb & lmask) + (uint32_t)h];
                uint32_t oi = wb * (uint32_t)nres + (uint32_t)h;                  // out[(w * n_res + r) * H + h], r = 0
                double o0 = 0.0, o1 = 0.0;
                if (nres > 0) o0 = rout[oi];                                      // wave-uniform tests
                if (nres > 1) o1 = rout[oi + (uint32_t)H];
                double cap = 0.0;
                for (int q = 0; q < nw; ++q) {
                    const uint32_t up = ~seg[q][i];
                    const int kn = ngen - 32 * q < 32 ? ngen - 32 * q : 32;
                    for (int b = 0; b < kn; ++b) cap += ((up >> b) & 1u) ? S->cap[32 * q + b] : 0.0;   // ascending units; + 0.0 is exact
                }
                if (nres > 0) cap = hl1_var_add(cap, A.rscale[0], o0);
                if (nres > 1) cap = hl1_var_add(cap, A.rscale[1], o1);
                for (int r = 2; r < nres; r += 2) {                               // the others two at a time: one wait per pair
                    const uint32_t oj = oi + (uint32_t)r * (uint32_t)H;
                    const bool two = r + 1 < nres;
                    const double a = rout[oj], b = two ? rout[oj + (uint32_t)H] : 0.0;
                    cap = hl1_var_add(cap, A.rscale[r], a);
                    if (two) cap = hl1_var_add(cap, A.rscale[r + 1], b);
                }
                const double L = hl1_storage_load(A.scale, ld, A.shift);
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
