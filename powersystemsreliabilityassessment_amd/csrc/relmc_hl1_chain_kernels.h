// relmc_hl1_chain_kernels.h — the HL1 sequential chronology of one area (PowerSystemAdequacy.jl:214-268; contracts in include/relmc.h) in
// its four models, as one kernel template:
//   sequential   relmc_hl1_seq: loss hours, EUE and loss events of every chain year
//   events       relmc_hl1_seq_events: a loss event is a maximal run of consecutive loss steps of a chain; every event's start step,
//                duration, energy and peak, the per-chain summary records and the duration histogram (the kernels that scan the
//                counts and reduce the records in a fixed order are relmc_seq_kernels.h's)
//   sweep        relmc_hl1_seq_sweep: one walk of a chain's fleet history compared with up to RELMC_HL1_SWEEP_MAX_LEVELS load levels
//                L_j(h) = scale_j * load[h] + shift_j, each against the whole fleet or the fleet without the withheld units
//   maintenance  relmc_hl1_maint_seq: one walk compared with up to RELMC_HL1_MAINT_MAX_SCHEDULES maintenance schedules.  A unit on
//                maintenance under schedule j in an hour adds 0.0 to that hour's capacity of schedule j; its failure and repair
//                process runs on
// The events, the sweep and the maintenance are extensions beyond the reference (PowerSystemAdequacy.jl has one load curve and no event
// list; generating_adequancy_comparative.jl has the overlay rule, on independently drawn hours).
// Only the template and inline functions are defined here, and nothing is instantiated: a unit that includes this header holds the
// instantiations it launches and no other kernel (relmc_seq.hip the first three models', relmc_maint.hip the fourth's).
#pragma once
#include <type_traits>
#include <utility>
#include "../../include/relmc.h"
#include "relmc_devfn.h"
#include "relmc_hl1_chrono.h"

namespace relmc {

// ---- sequential model -----------------------------------------------------------------------------------------------------------------
// The wave's open year: fixed-order butterfly over the lanes' partials, lane 0 stores (lole, eue, lolf); the partials restart at zero
DEVFI void hl1_seq_close_year(double& l, double& e, double& f, double* __restrict__ out)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { l += __shfl_xor(l, off); e += __shfl_xor(e, off); f += __shfl_xor(f, off); }
    if ((threadIdx.x & 63) == 0) { out[0] = l; out[1] = e; out[2] = f; }
    l = e = f = 0.0;
}

// ---- event model ----------------------------------------------------------------------------------------------------------------------
// Lane `src`'s value (src wave-uniform) / a value that is the same in every lane, moved into scalar registers: the carry and the chain's
// record are wave-uniform, and held this way they cost no vector register (the event model keeps the sequential model's occupancy)
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

// ---- sweep and maintenance models: one record row per level / per schedule -----------------------------------------------------------
// The levels and the withheld-unit mask, passed BY VALUE as a kernel argument: every read of a level is a scalar load from the kernel
// argument segment, and the per-level branches are wave-uniform
struct Hl1SweepArgs {
    relmc_hl1_sweep_level lv[RELMC_HL1_SWEEP_MAX_LEVELS];
    uint32_t withheld[4];                                    // bit k & 31 of word k >> 5: unit k is not part of fleet 1
    int32_t n_levels;
    uint32_t fleet1;                                         // bit j: level j uses fleet 1 (lv[j].fleet, gathered by the host)
};
// The host fills lv[n_levels ..] with levels that never lose (scale 0, shift -inf: L = -inf, and no capacity is below it), so the passes
// over the levels need no test against n_levels; only the year records are written for j < n_levels alone.

// A row of the records is a level of the sweep or a schedule of the maintenance model; NR = the instantiation's row count.
// f(integral_constant<int, j>) for j = 0 .. NR - 1, written out at compile time: a row's registers are named by a constant.  (A
// `#pragma unroll` loop with the run-time exit at n_levels was left a loop at NR = 16, and the partials were then indexed at run time.)
template <class F, int... J>
DEVFI void hl1_rows_each(F&& f, std::integer_sequence<int, J...>) { (f(std::integral_constant<int, J>{}), ...); }
template <int NR, class F>
DEVFI void hl1_rows(F&& f) { hl1_rows_each(f, std::make_integer_sequence<int, NR>{}); }

// The wave's open year of every row: loss hours and events are wave-uniform counts, row j's in lane j of cL / cF (32 scalar registers
// as arrays: 391 scalar spills at 16 levels); EUE is the sequential model's fixed-order butterfly
// over the lanes' partials (hl1_seq_close_year) -- skipped for a row without a loss hour in the year, whose partials are all +0.0 and
// sum to +0.0 in any order.  Lane 0 stores (lole, eue, lolf) at out + j * row_stride; the counts and partials restart at zero.
template <int NR>
DEVFI void hl1_rows_close_year(int nr, uint32_t& cL, uint32_t& cF, double (&aE)[NR], double* __restrict__ out, size_t row_stride)
{
    hl1_rows<NR>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        if (j < nr) {                                        // wave-uniform
            const uint32_t l = (uint32_t)__builtin_amdgcn_readlane((int)cL, j), f = (uint32_t)__builtin_amdgcn_readlane((int)cF, j);
            double e = 0.0;
            if (l != 0u) {                                   // wave-uniform
                e = aE[j];
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) e += __shfl_xor(e, off);
                aE[j] = 0.0;
            }
            if ((threadIdx.x & 63) == 0) { double* const o = out + (size_t)j * row_stride; o[0] = (double)l; o[1] = e; o[2] = (double)f; }
        }
    });
    cL = 0u; cF = 0u;
}

// ---- the kernel template --------------------------------------------------------------------------------------------------------------
enum Hl1ChainModel : int { HL1_CHAIN_SEQ, HL1_CHAIN_EVENTS, HL1_CHAIN_SWEEP, HL1_CHAIN_MAINT };

// What a model's kernel takes after `start`.  These are kernel parameters of their own (the template's pack) and not one by-value struct:
// a pointer read out of a struct is not __restrict__ to the compiler, and the argument segments stay those the four kernels had.
template <int MODEL> struct Hl1ChainTail;
template <> struct Hl1ChainTail<HL1_CHAIN_SEQ> {
    double* __restrict__ year_out;                           // year_out[chain of the launch][year][3]
};
template <> struct Hl1ChainTail<HL1_CHAIN_EVENTS> {
    int32_t n_bins;
    unsigned long long* __restrict__ hist;
    Hl1EventRec* __restrict__ rec;
    long long* __restrict__ count;
    const long long* __restrict__ offset;
    int64_t chain_base, cap;
    relmc_hl1_event* __restrict__ events;
};
template <> struct Hl1ChainTail<HL1_CHAIN_SWEEP> {
    const Hl1SweepArgs& A;
    double* __restrict__ year_out;                           // year_out[level][chain of the launch][year][3]
};
template <> struct Hl1ChainTail<HL1_CHAIN_MAINT> {
    double scale, shift;                                     // the one load of all schedules: scale * load[h] + shift
    int32_t n_sched;
    const uint32_t* __restrict__ tab;                        // tab[schedule][hour of the year][4], P schedules
    double* __restrict__ year_out;                           // year_out[schedule][chain of the launch][year][3]
};

// A variable that only some of the template's instantiations have: T where ON, elsewhere an empty object.  Either starts from `{}` (zero,
// false, nullptr): an empty object built from an initialiser, or one declared in the step loop, changed the other models' code.
struct Hl1Absent {};
template <bool ON, class T> using Hl1Only = std::conditional_t<ON, T, Hl1Absent>;

// Chain c = blockIdx.x * 4 + wave.  Lane l owns units l and l + 64; its cursor (state, next transition time, next draw) stays in
// registers for the whole chain.  The chain advances in windows of HL1_SEQ_WINDOW steps: (1) the down intervals reaching into the
// window are filled into the wave's LDS masks by the whole wave, 64 steps per instruction, one interval at a time (each lane touches
// its own step, so a plain OR is race-free); (2) one step per lane: capacity of the UP units in ascending unit order, then what the model
// does with the group's capacities.  No workgroup barrier: the four waves run four chains.
//
// The four models are instantiations of this one text (MODEL; P = LIST for the events, the row count for the sweep (NL levels) and the
// maintenance (NS schedules); ARG = the members of Hl1ChainTail<MODEL>, in order and with their __restrict__), each with the instructions
// it had as a kernel of its own: the prologue, the cursor start, the window clear, stage (1), the step index with its hour / year walk
// and the capacity sum are written once, a model's state (declared through Hl1Only, so that no instantiation holds another model's;
// what the sweep and the maintenance have in common, the rows' state, once for both), its stage and its tail are under `if constexpr`.
// The *kernel* is the template, on purpose.  The window loop is not a function that the kernels call: the two attempts to share it that
// way each cost the sequential model 1.6-3 %, with any of the start rule, the fill or the cursor in a function of its
// own, while the template route gives the compiler each kernel's whole text as before.  DESIGN.md 6.12 lists the formulations of this
// text that did not reproduce the kernels' code.  The kernels of the other tracks (storage, multi-state, multi-area) keep a window
// loop of their own for the same reason.
//
// sequential  loss flag and deficit against load[(n-1) mod H], rising edge (the previous step's flag from the neighbouring lane, lane 63's
//   carried over), and the lane partials of the open year, closed by a fixed-order reduction when a later year appears.
//   Records: year_out[chain][year][3].
//
// events  m = ballot of the lanes' loss flags.  A flagged (segmented) scan over the lanes gives every loss lane the
//   deficit sum and maximum of its run from the run's first lane of the group on (6 steps; a lane's run starts behind the highest clear
//   bit of m below it).  A lane whose successor has no loss closes its run and owns the event; a run that reaches lane 63 stays open in the
//   wave-uniform carry (open, start step, duration, energy, peak), which crosses groups, windows and years and is closed by the first
//   later group whose lane 0 has no loss, or by the chain's last step (censored).  Closing lanes are ranked by the ballot, so a chain's
//   events are numbered in step order; the chain's record takes them one by one in that order, wave-uniform in scalar registers (a
//   per-lane record cost 18 vector registers and with them one wave per SIMD: +3.7 % on the sequential model's time instead of -5 %).
//   Groups without a loss step and without an open run (nearly all of them) skip all of this.
//     LIST = false: per-chain summary record rec[chain], event count count[chain], duration histogram hist[n_bins] (integer atomics)
//     LIST = true:  event j of the chain goes to events[offset[chain] + j] if that index is below cap; nothing else is written
//
// sweep  per step the lane forms cap (every UP unit) and, if a level uses fleet 1, cap1 (a withheld unit adds 0.0) in the one ascending
//   loop over the mask bits.  A first pass over the levels forms only the ballots of the loss flags: a 64-step group in which no level has a
//   loss step and no level's flag was up on the step before does nothing further (nearly all groups).  Otherwise each level that has a loss
//   step or an open flag takes: loss hours and rising edges by popcount of the ballots restricted to the lanes of the open year, the
//   deficit into the lane's fp64 partial of the level (the sequential model's order: the lane's steps of the year ascending, + 0.0 left
//   out), and its bit of the wave-uniform previous-step mask.  Years are closed when a later year shows up in an active group, or at the
//   end of the chain; a skipped group adds nothing, so closing late changes no sum.  The passes over the levels are written out at compile
//   time (hl1_rows), so no register array is indexed at run time.  Records: year_out[level][chain of the launch][year][3].
//
// maintenance  tab[schedule][hour of the year][4]: bit k & 31 of word k >> 5 = unit k on maintenance.  The table holds NS schedules (the
//   host adds empty ones above n_sched) and no bit at or above ngen.  Per step the lane reads its hour's words of each schedule --
//   consecutive lanes read consecutive hours, 16 bytes apart, so a wave's read of a schedule is one contiguous kilobyte -- and forms
//   cap_j for the NS schedules in ONE ascending loop over the units: a unit's capacity is one scalar load for all schedules, and unit k
//   adds cap_k to cap_j where its bit of (UP & ~maintenance_j) is set, 0.0 elsewhere.  With more than one schedule a first pass over the
//   words asks whether any lane of the group has an UP unit on maintenance under any schedule; if none has, every cap_j is the one sum
//   over the UP units (a unit that is DOWN adds 0.0 with or without maintenance, so the bits are those of the ascending sum).  From there
//   on it is the sweep's stage with schedules for levels, cap_j for the level's fleet and one load L = scale * load[h] + shift for every
//   schedule.  Records: year_out[schedule][chain of the launch][year][3].
template <int MODEL, int P, class... ARG>
__global__ void __launch_bounds__(256) relmc_hl1_chain_kernel(const Hl1SeqCase* __restrict__ S, const double* __restrict__ load, uint64_t seed,
                                                              uint64_t first_chain, int64_t n_chains, int32_t years, int32_t start, ARG... arg)
{
    constexpr bool SEQ = MODEL == HL1_CHAIN_SEQ, EVENTS = MODEL == HL1_CHAIN_EVENTS, SWEEP = MODEL == HL1_CHAIN_SWEEP, MAINT = MODEL == HL1_CHAIN_MAINT;
    constexpr bool LIST = EVENTS && P != 0;
    constexpr bool ROWS = SWEEP || MAINT;                    // one record row per level / per schedule
    constexpr int NR = ROWS ? P : 1;
    constexpr int W = HL1_SEQ_WINDOW;
    __shared__ uint32_t masks[4][4][W];                     // [wave][mask word][step of the window], bit k & 31 of word k >> 5 = unit k down
    const Hl1ChainTail<MODEL> T{arg...};
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t cl = (int64_t)blockIdx.x * 4 + wv;
    if (cl >= n_chains) return;                              // wave-uniform
    Hl1Only<EVENTS, long long> off0{};                       // LIST: the chain's first index in the caller's list
    if constexpr (LIST) {
        off0 = T.offset[cl];
        if (off0 >= T.cap) return;                           // the caller's list is full before this chain (wave-uniform)
    }
    const uint64_t chain = first_chain + (uint64_t)cl;
    const int ngen = S->ngen, H = S->nhours, nw = (ngen + 31) >> 5, nslot = ngen > 64 ? 2 : 1;
    Hl1Only<ROWS, int> nr{};                                 // rows that are written: the caller's levels / schedules, NR at the most
    Hl1Only<SWEEP, bool> use1{};                             // some level uses fleet 1
    if constexpr (SWEEP) { nr = T.A.n_levels < NR ? T.A.n_levels : NR; use1 = T.A.fleet1 != 0u; }
    if constexpr (MAINT) nr = T.n_sched < NR ? T.n_sched : NR;
    uint32_t (*const seg)[W] = masks[wv];
    const int64_t nsteps = (int64_t)years * H;
    Hl1Only<ROWS, size_t> row_stride{};
    if constexpr (ROWS) row_stride = (size_t)n_chains * (size_t)years * 3;
    Hl1Only<!EVENTS, double*> out{};                         // the chain's year records (with rows: of row 0)
    if constexpr (!EVENTS) out = T.year_out + (size_t)cl * (size_t)years * 3;

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

    // sequential: this lane's partials of the open year ycur
    Hl1Only<SEQ, double> aL{}, aE{}, aF{};
    // events
    Hl1Only<EVENTS, Hl1EventRec> a;                          // the chain's record so far (wave-uniform, events = cnt at the end)
    if constexpr (EVENTS) hl1_event_rec_zero(a);
    Hl1Only<EVENTS, long long> cnt{};                        // events closed so far (wave-uniform)
    Hl1Only<EVENTS, bool> open{};                            // wave-uniform carry: a run that reached the last step before the group
    Hl1Only<EVENTS, long long> cn0{}, cD{};
    Hl1Only<EVENTS, double> cE{}, cP{};
    // (the three lambdas stand here and not in the step stage, where they exchanged two of its instructions; only the event model's
    // instantiations give them a body)
    // LIST: the event (n0, D, E, P), number j of the chain, stored by the lane that owns it
    auto store = [&](long long n0, long long D, double E, double Pk, long long j) {
        if constexpr (EVENTS) {
            const long long at = off0 + j;
            if (at < T.cap) {
                relmc_hl1_event* const e = T.events + at;
                e->chain = T.chain_base + cl; e->start_step = n0; e->duration = D; e->energy_mwh = E; e->peak_mw = Pk;
            }
        }
    };
    // !LIST: one event into the chain's record, by the whole wave (every argument wave-uniform); events in step order
    auto account = [&](long long D, double E, double Pk, bool censored) {
        if constexpr (EVENTS) {
            a.sum_dur += D; a.sum_dur2 += D * D; a.max_dur = a.max_dur > D ? a.max_dur : D; a.censored += censored ? 1 : 0;
            a.sum_energy = hl1_event_uniform(a.sum_energy + E); a.sum_energy2 = hl1_event_uniform(__builtin_fma(E, E, a.sum_energy2));
            a.max_energy = hl1_event_uniform(fmax(a.max_energy, E)); a.max_peak = hl1_event_uniform(fmax(a.max_peak, Pk));
        }
    };
    auto count_dur = [&](long long D) {                      // !LIST: the histogram, by the lane that owns the event
        if constexpr (EVENTS) {
            if (T.hist) atomicAdd(T.hist + ((D < T.n_bins ? D : (long long)T.n_bins) - 1), 1ull);
        }
    };
    // sweep, maintenance
    Hl1Only<ROWS, double[NR]> aEl;                           // this lane's EUE partial of the open year ycur, per row
    Hl1Only<ROWS, uint32_t> cL{}, cF{};                      // the wave's loss hours and loss events of the open year: row j's in lane j
    if constexpr (ROWS) hl1_rows<NR>([&](auto jc) { aEl[decltype(jc)::value] = 0.0; });
    Hl1Only<!EVENTS, int> ycur{};
    Hl1Only<!EVENTS, int> gy{};                              // chain year and
    int gh = 0;                                              // hour of the year of the current 64-step group's first step
    Hl1Only<SEQ, bool> prev{};                               // loss flag of the step before the group (none before step 1)
    Hl1Only<ROWS, uint32_t> prevs{};                         // bit j: row j's loss flag on the step before the group (wave-uniform)
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
            int h = gh + lane, y = 0;                        // the step's hour of the year and chain year (the events tell no years apart)
            if constexpr (!EVENTS) y = gy;
            while (h >= H) { h -= H; if constexpr (!EVENTS) ++y; }
            bool f = false;                                  // sequential, events: the step's loss flag and deficit
            double d = 0.0;
            // cap: capacity of the UP units, summed here by the lanes with a step; in the sweep by every lane, or, with a level on fleet 1,
            // by none: its stage below then forms both fleets' capacities in one loop; never in the maintenance model, whose stage forms
            // its schedules' capacities.  (One text for both loops did not hold: as a lambda or a function over F1 it exchanged two
            // register pairs of the sequential model's year close, and with the fleet test inside this loop the sweep lost the two loops
            // it had.)
            double cap = 0.0;
            bool plain = valid;
            if constexpr (SWEEP) plain = !use1;              // wave-uniform
            if constexpr (MAINT) plain = false;
            if (plain) {
                for (int q = 0; q < nw; ++q) {
                    const uint32_t up = ~seg[q][i];
                    const int kn = ngen - 32 * q < 32 ? ngen - 32 * q : 32;
                    for (int b = 0; b < kn; ++b) cap += ((up >> b) & 1u) ? S->cap[32 * q + b] : 0.0;   // ascending units; + 0.0 is exact
                }
                if constexpr (!SWEEP) {
                    const double ld = load[h];
                    f = cap < ld;
                    d = f ? ld - cap : 0.0;
                }
            }
            if constexpr (SEQ) {
                const int fl = __shfl_up((int)f, 1);
                const bool r = f && !(lane == 0 ? prev : fl != 0);
                prev = __shfl((int)f, 63) != 0;
                for (;;) {
                    if (valid && y == ycur) { aL += f ? 1.0 : 0.0; aE += d; aF += r ? 1.0 : 0.0; }
                    if (!__any(valid && y > ycur)) break;
                    hl1_seq_close_year(aL, aE, aF, out + (size_t)ycur * 3);
                    ++ycur;
                }
            }
            if constexpr (EVENTS) {
                const uint64_t m = __ballot(f);                  // lanes past the chain's last step carry no loss
                if (m != 0 || open) {                         // wave-uniform
                    const int64_t base = w0 + g;                 // step of lane 0
                    if (open && !(m & 1)) {                   // the open run ended with the step before the group
                        if constexpr (LIST) { if (lane == 0) store(cn0, cD, cE, cP, cnt); }
                        else { account(cD, cE, cP, false); if (lane == 0) count_dur(cD); }
                        ++cnt; open = false;
                    }
                    if (m != 0) {
                        const uint64_t z = ~m & ((1ull << lane) - 1);
                        const int s0 = z ? 64 - __builtin_clzll(z) : 0;               // first lane of this lane's run in the group
                        double rs = d, rp = d;
#pragma unroll
                        for (int o = 1; o < 64; o <<= 1) {
                            const double vs = __shfl_up(rs, o), vp = __shfl_up(rp, o);
                            if (lane - o >= s0) { rs = vs + rs; rp = fmax(vp, rp); }
                        }
                        const bool end63 = base + 63 == nsteps;                       // lane 63 is the chain's last step: its run ends there
                        uint64_t c = m & ~(m >> 1);
                        if (!end63) c &= ~(1ull << 63);
                        const bool cont = open && s0 == 0;                         // the run came in through the carry
                        const long long n0 = cont ? cn0 : base + s0, D = (cont ? cD : 0) + (lane - s0 + 1);
                        const double E = cont ? cE + rs : rs, Pk = cont ? fmax(cP, rp) : rp;
                        if constexpr (LIST) {
                            if ((c >> lane) & 1) store(n0, D, E, Pk, cnt + __popcll(c & ((1ull << lane) - 1)));
                        } else {
                            if ((c >> lane) & 1) count_dur(D);
                            for (uint64_t cc = c; cc; cc &= cc - 1) {                 // ascending lanes = step order
                                const int src = __builtin_ctzll(cc);
                                account(hl1_event_lane(D, src), hl1_event_lane(E, src), hl1_event_lane(Pk, src), base + src == nsteps);
                            }
                        }
                        cnt += __popcll(c);
                        if ((m >> 63) && !end63) {                                    // lane 63's run goes on into the next group
                            const int st63 = __builtin_amdgcn_readlane(s0, 63);
                            const double s63 = hl1_event_lane(rs, 63), p63 = hl1_event_lane(rp, 63);
                            if (open && st63 == 0) { cD += 64; cE = hl1_event_uniform(cE + s63); cP = hl1_event_uniform(fmax(cP, p63)); }
                            else { cn0 = base + st63; cD = 64 - st63; cE = s63; cP = p63; open = true; }
                        } else open = false;
                    }
                }
            }
            if constexpr (SWEEP) {
                const Hl1SweepArgs& A = T.A;
                double cap1 = 0.0;                               // fleet 1: a withheld unit adds 0.0
                if (use1) {                                      // wave-uniform: cap and cap1 in the one ascending loop
                    for (int q = 0; q < nw; ++q) {
                        const uint32_t up = ~seg[q][i], wh = A.withheld[q];
                        const int kn = ngen - 32 * q < 32 ? ngen - 32 * q : 32;
                        for (int b = 0; b < kn; ++b) {
                            const double c = S->cap[32 * q + b], c1 = ((wh >> b) & 1u) ? 0.0 : c;
                            cap += ((up >> b) & 1u) ? c : 0.0;
                            cap1 += ((up >> b) & 1u) ? c1 : 0.0;
                        }
                    }
                }
                const double ld = load[h];
                // which levels have a loss step in the group (the comparison's lane mask is the ballot)
                uint32_t act = prevs;
                // a level's scale, shift and fleet bit are read where they are used (z is a zero the compiler cannot see through): read once
                // before the loops they are some 100 scalar registers live across the whole chain, most of them spilled to vector lanes
                int z = 0;
                __asm__ volatile("" : "+s"(z));
                const uint32_t fleet1 = A.fleet1 | (uint32_t)z;
                hl1_rows<NR>([&](auto jc) {
                    constexpr int j = decltype(jc)::value;
                    const double L = hl1_sweep_load(A.lv[j + z].scale, ld, A.lv[j + z].shift);
                    const double cj = ((fleet1 >> j) & 1u) ? cap1 : cap;
                    if (__builtin_amdgcn_ballot_w64(valid && cj < L) != 0) act |= 1u << j;
                });
                if (act != 0u) {                                 // wave-uniform
                    // the levels' loads and flags are formed again from a copy of the load the compiler cannot see through: kept from the
                    // pass above they are 16 loads and 16 lane masks live across every group (167 vector registers, 323 scalar spills)
                    double lda = ld;
                    __asm__ volatile("" : "+v"(lda));
                    uint32_t next = 0u;
                    for (;;) {
                        const bool in = valid && y == ycur;
                        const uint64_t my = __builtin_amdgcn_ballot_w64(in);
                        next = 0u;
                        hl1_rows<NR>([&](auto jc) {
                            constexpr int j = decltype(jc)::value;
                            if ((act >> j) & 1u) {               // wave-uniform: a level without a loss step and without an open flag is left out
                                const double L = hl1_sweep_load(A.lv[j + z].scale, lda, A.lv[j + z].shift);
                                const double cj = ((fleet1 >> j) & 1u) ? cap1 : cap;
                                const bool fj = valid && cj < L;
                                const uint64_t m = __builtin_amdgcn_ballot_w64(fj);
                                const uint64_t r = m & ~((m << 1) | (uint64_t)((prevs >> j) & 1u));     // the flag rises: the step before had none
                                cL += lane == j ? (uint32_t)__popcll(m & my) : 0u; cF += lane == j ? (uint32_t)__popcll(r & my) : 0u;
                                aEl[j] += (fj && in) ? L - cj : 0.0;
                                next |= (uint32_t)(m >> 63) << j;
                            }
                        });
                        if (!__any(valid && y > ycur)) break;
                        hl1_rows_close_year<NR>(nr, cL, cF, aEl, out + (size_t)ycur * 3, row_stride);
                        ++ycur;
                    }
                    prevs = next;
                }
            }
            if constexpr (MAINT) {
                const uint32_t* const mrow = T.tab + (size_t)h * 4;                   // schedule j's words of the hour: mrow[j * H * 4 + q]
                const size_t sched_words = (size_t)H * 4;
                double capj[NR];
                hl1_rows<NR>([&](auto jc) { capj[decltype(jc)::value] = 0.0; });
                bool overlay = true;                             // wave-uniform: some lane has an UP unit on maintenance under some schedule
                if constexpr (NR > 1) {
                    uint32_t hit = 0u;
                    for (int q = 0; q < nw; ++q) {
                        const uint32_t up = ~seg[q][i];
                        hl1_rows<NR>([&](auto jc) { hit |= up & mrow[(size_t)decltype(jc)::value * sched_words + q]; });
                    }
                    overlay = __builtin_amdgcn_ballot_w64(valid && hit != 0u) != 0;
                }
                if (overlay) {
                    for (int q = 0; q < nw; ++q) {
                        const uint32_t up = ~seg[q][i];
                        uint32_t on[NR];                         // UP and not on maintenance under schedule j
                        hl1_rows<NR>([&](auto jc) {
                            constexpr int j = decltype(jc)::value;
                            on[j] = up & ~mrow[(size_t)j * sched_words + q];
                        });
                        const int kn = ngen - 32 * q < 32 ? ngen - 32 * q : 32;
                        for (int b = 0; b < kn; ++b) {
                            const double c = S->cap[32 * q + b];
                            hl1_rows<NR>([&](auto jc) {                               // ascending units; + 0.0 is exact
                                constexpr int j = decltype(jc)::value;
                                capj[j] += ((on[j] >> b) & 1u) ? c : 0.0;
                            });
                        }
                    }
                } else {
                    double all = 0.0;
                    for (int q = 0; q < nw; ++q) {
                        const uint32_t up = ~seg[q][i];
                        const int kn = ngen - 32 * q < 32 ? ngen - 32 * q : 32;
                        for (int b = 0; b < kn; ++b) all += ((up >> b) & 1u) ? S->cap[32 * q + b] : 0.0;
                    }
                    hl1_rows<NR>([&](auto jc) { capj[decltype(jc)::value] = all; });
                }
                const double L = hl1_sweep_load(T.scale, load[h], T.shift);
                // which schedules have a loss step in the group (the comparison's lane mask is the ballot)
                uint32_t act = prevs;
                hl1_rows<NR>([&](auto jc) {
                    constexpr int j = decltype(jc)::value;
                    if (j < nr && __builtin_amdgcn_ballot_w64(valid && capj[j] < L) != 0) act |= 1u << j;
                });
                // The sweep's account of the group, with the one L and capj[j] for the level's load and fleet.  It is written a second time:
                // as one text for both models (a lambda over the row's load and capacity, or one loop with the models' values declared
                // ahead of it) it did not reproduce the sweep's or the maintenance kernels' code.
                if (act != 0u) {                                 // wave-uniform
                    uint32_t next = 0u;
                    for (;;) {
                        const bool in = valid && y == ycur;
                        const uint64_t my = __builtin_amdgcn_ballot_w64(in);
                        next = 0u;
                        hl1_rows<NR>([&](auto jc) {
                            constexpr int j = decltype(jc)::value;
                            if ((act >> j) & 1u) {               // wave-uniform: a schedule without a loss step and without an open flag is left out
                                const bool fj = valid && capj[j] < L;
                                const uint64_t m = __builtin_amdgcn_ballot_w64(fj);
                                const uint64_t r = m & ~((m << 1) | (uint64_t)((prevs >> j) & 1u));     // the flag rises: the step before had none
                                cL += lane == j ? (uint32_t)__popcll(m & my) : 0u; cF += lane == j ? (uint32_t)__popcll(r & my) : 0u;
                                aEl[j] += (fj && in) ? L - capj[j] : 0.0;
                                next |= (uint32_t)(m >> 63) << j;
                            }
                        });
                        if (!__any(valid && y > ycur)) break;
                        hl1_rows_close_year<NR>(nr, cL, cF, aEl, out + (size_t)ycur * 3, row_stride);
                        ++ycur;
                    }
                    prevs = next;
                }
            }
            gh += 64;
            while (gh >= H) { gh -= H; if constexpr (!EVENTS) ++gy; }
        }
        hl1_seq_wave_sync();
    }
    if constexpr (SEQ) hl1_seq_close_year(aL, aE, aF, out + (size_t)ycur * 3);
    if constexpr (EVENTS && !LIST) {
        if (lane == 0) { a.events = cnt; T.rec[cl] = a; T.count[cl] = cnt; }
    }
    if constexpr (ROWS)
        for (; ycur < years; ++ycur) hl1_rows_close_year<NR>(nr, cL, cF, aEl, out + (size_t)ycur * 3, row_stride);
}
// The eleven instantiations go by the names relmc_hl1_seq_kernel, relmc_hl1_event_kernel<LIST>, relmc_hl1_sweep_kernel<NL>
// (relmc_seq.hip) and relmc_hl1_maint_kernel<NS> (relmc_maint.hip), each defined in the unit that launches it: a name defined here
// that is no template would instantiate its kernel in every unit that reads this header.
}  // namespace relmc
