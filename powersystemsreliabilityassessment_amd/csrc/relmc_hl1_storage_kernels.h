// relmc_hl1_storage_kernels.h — the HL1 sequential chronology with energy storage, in its three tracks (contracts in include/relmc.h), as
// one kernel template:
//   storage  relmc_hl1_seq_storage: one walk of a chain's fleet history against the load L(h) = scale * load[h] + shift, with up to
//            RELMC_HL1_MAX_STORAGE storages that discharge into a shortfall and charge from surplus generation
//   weather  relmc_hl1_var_seq: every chain year draws a weather year w of the library of relmc_hl1_var_load; the step's capacity is the
//            fleet's plus resource_scale[r] * output[w][r][h], its load scale * base(w, h) + shift
//   stress   relmc_hl1_stress_seq: the weather track, in which a UP unit of outage class c fails with the hazard
//            fail_mult[w(y)][c][h] / mttf in hour h of chain year y.  The time of a failure is no longer T + E: the draw E = -mttf * ln U is
//            spent along the cumulative multiplier table G of the unit's class, year by year (hl1_stress_failure_time, compiled for the
//            host and the device from this one text)
// All three are extensions beyond the reference: its only energy-limited resource, the ELU of the planning model, drains and never
// recharges, on an hourly-sampling Monte Carlo; its generation is all dispatchable; its units have constant rates.
// The weather pick, the storage step, the wave-uniform bits and the year close are relmc_hl1_storage_devfn.h's.
#pragma once
#include "relmc_hl1_chrono.h"
#include "relmc_hl1_storage_devfn.h"

namespace relmc {

// The contract's failure time (include/relmc.h, "Failure time"): a unit of a stressed class became UP at chain time T >= 0 and draws the
// hazard E > 0; -> the chain time at which it fails, or years * H + 1 when it does not fail within the chain.  row(y) is the cumulative
// table G[0 .. H] of the unit's class in the weather year of chain year y (0 <= y < years).  Every fp64 operation is rounded on its own
// (no contraction), so that the host, the device and the Python model of the tests give the same bits.
template <class Row>
__host__ __device__ inline double hl1_stress_failure_time(double T, double E, int H, int years, Row&& row)
{
#pragma clang fp contract(off)
    const double never = (double)((int64_t)years * H + 1);
    if (!(T < (double)((int64_t)years * H))) return T > never ? T : never;    // UP again at or after the chain's end: nothing to see
    const int64_t n0 = (int64_t)T;                           // floor: T >= 0
    int y = (int)(n0 / H), j = (int)(n0 - (int64_t)y * H);
    const double* G = row(y);
    const double frac = T - (double)n0;
    const double slope = G[j + 1] - G[j];
    const double part = slope * frac;
    double a = G[j] + part;
    double rem = G[H] - a;
    while (E > rem) {                                        // the year's hazard does not use the draw up
        E = E - rem;
        if (++y == years) return never;
        G = row(y);
        j = 0; a = 0.0; rem = G[H];
    }
    const double t = a + E;
    // The smallest j' in j .. H - 1 with G[j' + 1] >= t, H - 1 if there is none: at most ceil(log2 H) probes.  (A search that reads 15
    // pivots a level, 4 levels of independent loads, finds the same j' and was measured slower: DESIGN.md 6.10.)
    int lo = j, hi = H - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (G[mid + 1] >= t) hi = mid; else lo = mid + 1;
    }
    const double g0 = G[lo], d = G[lo + 1] - g0;
    double f = 1.0;
    if (d > 0.0) {
        const double num = t - g0;
        f = num / d;
        f = f < 0.0 ? 0.0 : f > 1.0 ? 1.0 : f;
    }
    const double r = (double)((int64_t)y * H + lo) + f;
    return r > T ? r : T;
}

// A track's model, passed BY VALUE as a kernel argument (as Hl1SweepArgs): every read of a field is a scalar load from the kernel argument
// segment, and the offsets of the fields are part of the code.  st[n_storage ..] and rscale[n_res ..] are zero and never read.
struct Hl1StorageArgs {                  // the storages and the load level
    relmc_hl1_storage st[RELMC_HL1_MAX_STORAGE];
    double scale, shift;
    int32_t n_storage, pad;
};
struct Hl1VarArgs {                      // and the resource scales and the weather library
    relmc_hl1_storage st[RELMC_HL1_MAX_STORAGE];
    double rscale[RELMC_HL1_VAR_MAX_RESOURCES];
    double scale, shift;
    const double* out;                   // [n_weather][n_res][H], fewer than 2^31 values (relmc_hl1_var_load): the kernel indexes it in 32 bits
    const double* wload;                 // [n_weather][H], or nullptr: the load curve of relmc_hl1_seq_load
    int32_t n_storage, n_res, n_weather, pick;
};
struct Hl1StressArgs {                   // and the stress library: the cumulative tables and the fleet's classes
    relmc_hl1_storage st[RELMC_HL1_MAX_STORAGE];
    double rscale[RELMC_HL1_VAR_MAX_RESOURCES];
    double scale, shift;
    const double* out;                   // as Hl1VarArgs
    const double* wload;
    const double* cum;                   // [n_weather][n_classes][H + 1], fewer than 2^31 values (relmc_hl1_stress_load)
    const int32_t* ucls;                 // [ngen]: -1 or a class
    int32_t n_storage, n_res, n_weather, pick, n_classes, reserved;
};

enum Hl1Track : int { HL1_TRACK_STORAGE, HL1_TRACK_WEATHER, HL1_TRACK_STRESS };
template <int TRACK> struct Hl1TrackArgs;
template <> struct Hl1TrackArgs<HL1_TRACK_STORAGE> { using type = Hl1StorageArgs; };
template <> struct Hl1TrackArgs<HL1_TRACK_WEATHER> { using type = Hl1VarArgs; };
template <> struct Hl1TrackArgs<HL1_TRACK_STRESS> { using type = Hl1StressArgs; };

// The kernel's setup reads a field that a track's struct lacks as nothing: no resources and no weather library, no classes
DEVFI int hl1_track_nres(const Hl1StorageArgs&) { return 0; }
DEVFI const double* hl1_track_wload(const Hl1StorageArgs&) { return nullptr; }
DEVFI const double* hl1_track_out(const Hl1StorageArgs&) { return nullptr; }
DEVFI int hl1_track_weather(const Hl1StorageArgs&, uint64_t, uint64_t, int, int) { return 0; }
template <class Args> DEVFI int hl1_track_nres(const Args& A) { return A.n_res < RELMC_HL1_VAR_MAX_RESOURCES ? A.n_res : RELMC_HL1_VAR_MAX_RESOURCES; }
template <class Args> DEVFI const double* hl1_track_wload(const Args& A) { return A.wload; }
template <class Args> DEVFI const double* hl1_track_out(const Args& A) { return A.out; }
template <class Args> DEVFI int hl1_track_weather(const Args& A, uint64_t seed, uint64_t chain, int y, int years) { return hl1_var_weather(seed, chain, y, years, A.n_weather, A.pick); }
template <class Args> DEVFI const double* hl1_track_cum(const Args&) { return nullptr; }
template <class Args> DEVFI uint32_t hl1_track_ncls(const Args&) { return 0u; }
DEVFI const double* hl1_track_cum(const Hl1StressArgs& A) { return A.cum; }
DEVFI uint32_t hl1_track_ncls(const Hl1StressArgs& A) { return (uint32_t)A.n_classes; }

// Chain c = blockIdx.x * 4 + wave; the chronology is relmc_hl1_seq_kernel's, word for word (lane l owns units l and l + 64, windows of
// HL1_SEQ_WINDOW steps filled into the wave's LDS masks, one step per lane, no workgroup barrier).  The window loop is written out here and
// not shared with relmc_hl1_seq_kernel (relmc_hl1_chain_kernels.h): sharing that loop between kernels as functions cost the
// sequential kernel 1.6-3 % twice.  The three tracks are instantiations of this one text, each with the instructions it had as a kernel of
// its own; what a track adds is under `if constexpr`, and the setup values a track has no use for are dead.
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
// The weather and stress tracks add to the parallel stage, one step per lane:
//   weather    a 64-step group may span several years when H < 64, so the weather year belongs to the lane's chain year y.  Each lane
//              keeps (yw, w * H) and works the pick out only when its y changes: once per lane and year, never per step
//   load       base(w, h) from the library's [w][h] curves or the sequential model's [h]: pointer and row mask chosen once per kernel
//   resources  cap = cap + rscale[r] * out[(w * n_res + r) * H + h] for r ascending, lanes on consecutive h (a lane past a year edge reads
//              another row), in 32-bit indices; the scales are scalar loads from the argument segment under wave-uniform tests; the first two
//              outputs and the load are read ahead of the capacity sum, the others in pairs
// The stress track adds to the transition of stage (1):
//   class      lane l keeps the classes of its units l and l + 64 in registers (cls[s], -1: the unit ignores the weather)
//   failure    a lane whose unit has just become UP and has a class runs hl1_stress_failure_time instead of the addition: a walk over the
//              years the draw outlasts (bounded by `years`; the weather year of each from hl1_var_weather), then a binary search of at
//              most ceil(log2 H) probes over one row of G in global memory, which every chain reads and L2 keeps.  These lanes diverge
//              from the others inside `while (__any(more))`; the loop's trip count is what it was, one trip per transition of the busiest lane
//   never      a unit that does not fail again gets years * H + 1, beyond every window: its cursor waits for the rest of the chain
// Records: year_out[row][chain of the launch][year][3], row 0 = (lole, eue, lolf), row 1 = (served_hours, discharged_mwh, charged_mwh).
// amdgpu_waves_per_eu: the stress track asks for (4, 4).  Left alone the allocator takes 131 VGPRs there, three waves per SIMD; asked for
// the weather track's four it finds 125 without scratch.  (1, 8) is what a kernel without the attribute gets.
template <int TRACK>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(TRACK == HL1_TRACK_STRESS ? 4 : 1, TRACK == HL1_TRACK_STRESS ? 4 : 8)))
relmc_hl1_storage_track_kernel(const Hl1SeqCase* __restrict__ S, const double* __restrict__ load, uint64_t seed, uint64_t first_chain, int64_t n_chains,
                               int32_t years, int32_t start, const typename Hl1TrackArgs<TRACK>::type A, double* __restrict__ year_out)
{
    constexpr bool WEATHER = TRACK != HL1_TRACK_STORAGE, STRESS = TRACK == HL1_TRACK_STRESS;
    constexpr int W = HL1_SEQ_WINDOW;
    constexpr int NS = RELMC_HL1_MAX_STORAGE;
    __shared__ uint32_t masks[4][4][W];                     // [wave][mask word][step of the window], bit k & 31 of word k >> 5 = unit k down
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t cl = (int64_t)blockIdx.x * 4 + wv;
    if (cl >= n_chains) return;                              // wave-uniform
    const uint64_t chain = first_chain + (uint64_t)cl;
    const int ngen = S->ngen, H = S->nhours, nw = (ngen + 31) >> 5, nslot = ngen > 64 ? 2 : 1;
    const int ns = A.n_storage < NS ? A.n_storage : NS;
    const int nres = hl1_track_nres(A);
    const double* __restrict__ const lcurve = hl1_track_wload(A) ? hl1_track_wload(A) : load;    // base(w, h) = lcurve[(w * H & lmask) + h]
    const uint32_t lmask = hl1_track_wload(A) ? ~0u : 0u;
    const double* __restrict__ const rout = hl1_track_out(A);
    const double* __restrict__ const cum = hl1_track_cum(A);
    const uint32_t ncls = hl1_track_ncls(A), H1 = (uint32_t)H + 1u;
    uint32_t (*const seg)[W] = masks[wv];
    const int64_t nsteps = (int64_t)years * H;
    double* const out0 = year_out + (size_t)cl * (size_t)years * 3;
    double* const out1 = out0 + (size_t)n_chains * (size_t)years * 3;

    bool down[2], mine[2];
    double tn[2], mf[2], mr[2];
    int ev[2], cls[2];
    int64_t since[2];
    // the failure time of a unit of class c that became UP at T with the draw E (c >= 0; G's row of (w, c) starts at (w * ncls + c) * (H + 1))
    auto fail_at = [&](double T, double E, int c) {
        return hl1_stress_failure_time(T, E, H, years, [&](int y) {
            return cum + ((uint32_t)hl1_track_weather(A, seed, chain, y, years) * ncls + (uint32_t)c) * H1;
        });
    };
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int k = lane + 64 * s;
        mine[s] = k < ngen;
        mf[s] = mine[s] ? S->mttf[k] : 1.0; mr[s] = mine[s] ? S->mttr[k] : 1.0;
        if constexpr (STRESS) cls[s] = mine[s] ? A.ucls[k] : -1;
        else cls[s] = -1;
        down[s] = false; ev[s] = 0; since[s] = 1; tn[s] = 0.0;
        if (mine[s]) {
            if (start == RELMC_HL1_START_STATIONARY) { down[s] = hl1_seq_u(chain, k, 0, seed) < S->q[k]; ev[s] = 1; }
            const double e = __dmul_rn(-(down[s] ? mr[s] : mf[s]), log(hl1_seq_u(chain, k, ev[s], seed)));    // T_1 = 0 + duration, or
            tn[s] = (STRESS && !down[s] && cls[s] >= 0) ? fail_at(0.0, e, cls[s]) : e;                           // the failure time from 0
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
                        const double e = __dmul_rn(-(down[s] ? mr[s] : mf[s]), l);
                        if (STRESS && !down[s] && cls[s] >= 0) tn[s] = fail_at(tn[s], e, cls[s]);   // UP in a stressed class: the hazard along G
                        else tn[s] = __dadd_rn(tn[s], e);                         // no FMA: the host model rounds the same way
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
                double ld = 0.0, o0 = 0.0, o1 = 0.0;
                uint32_t oi = 0u;
                if constexpr (WEATHER) {
                    if (y != yw) { yw = y; wb = (uint32_t)hl1_track_weather(A, seed, chain, y, years) * (uint32_t)H; }
                    // the step's load and its first two outputs are read BEFORE the capacity sum, whose work hides their latency
                    ld = lcurve[(wb & lmask) + (uint32_t)h];
                    oi = wb * (uint32_t)nres + (uint32_t)h;                       // out[(w * n_res + r) * H + h], r = 0
                    if (nres > 0) o0 = rout[oi];                                  // wave-uniform tests
                    if (nres > 1) o1 = rout[oi + (uint32_t)H];
                }
                double cap = 0.0;
                for (int q = 0; q < nw; ++q) {
                    const uint32_t up = ~seg[q][i];
                    const int kn = ngen - 32 * q < 32 ? ngen - 32 * q : 32;
                    for (int b = 0; b < kn; ++b) cap += ((up >> b) & 1u) ? S->cap[32 * q + b] : 0.0;   // ascending units; + 0.0 is exact
                }
                double L;
                if constexpr (WEATHER) {
                    if (nres > 0) cap = hl1_var_add(cap, A.rscale[0], o0);
                    if (nres > 1) cap = hl1_var_add(cap, A.rscale[1], o1);
                    for (int r = 2; r < nres; r += 2) {                           // the others two at a time: one wait per pair
                        const uint32_t oj = oi + (uint32_t)r * (uint32_t)H;
                        const bool two = r + 1 < nres;
                        const double a = rout[oj], b = two ? rout[oj + (uint32_t)H] : 0.0;
                        cap = hl1_var_add(cap, A.rscale[r], a);
                        if (two) cap = hl1_var_add(cap, A.rscale[r + 1], b);
                    }
                    L = hl1_storage_load(A.scale, ld, A.shift);
                } else L = hl1_storage_load(A.scale, load[h], A.shift);
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
