// relmc_dev.h — device-side view of one study case (built on the host by relmc_case_load,
// resident in HBM, copied into LDS by every workgroup) and the tile constants the gfx950
// kernels are compiled for.
#pragma once
#include <stdint.h>

namespace relmc {

// ---- tile geometry: one scenario = one row of RW lanes of a wavefront (64 / RW scenarios per wavefront) -----
//   Tile24: 16-lane DPP rows, 4 scenarios per wavefront  (<= 32 buses, 48 lines, 64 injections: IEEE RTS-24)
//   Tile96: one scenario per wavefront                   (<= 128 buses, 128 lines, 192 injections: IEEE RTS-96)
template <int RW_, int BS_, int LS_, int IS_, int NCOMPMAX_, int MAXPASS_, int MAXOFF_, int WPB_>
struct TileT {
    static constexpr int RW = RW_;             // lanes per scenario
    static constexpr int BS = BS_;             // bus slots per lane
    static constexpr int LS = LS_;             // line slots per lane
    static constexpr int IS = IS_;             // injection slots per lane
    static constexpr int NBT = BS_ * RW_;
    static constexpr int NLT = LS_ * RW_;
    static constexpr int NIT = IS_ * RW_;
    static constexpr int SPW = 64 / RW_;       // scenarios per wavefront
    static constexpr int NCOMPMAX = NCOMPMAX_; // sampled components (generators + lines)
    static constexpr int OW = NCOMPMAX_ / 32;  // 32-bit words of the outage mask
    static constexpr int MAXPASS = MAXPASS_;   // passes of the static solver schedule
    static constexpr int MAXOFF = MAXOFF_;     // off-diagonal 2x2 blocks of the factor (lines + fill)
    static constexpr int WPB = WPB_;           // wavefronts per workgroup (they share the case tables)
    static_assert(BS_ <= 2 && LS_ <= 3 && IS_ <= 4, "the per-lane flag word has room for 2 bus, 3 line and 4 injection slots");
};
using Tile24 = TileT<16, 2, 3, 4, 128, 96, 160, 4>;
using Tile96 = TileT<64, 2, 2, 3, 256, 64, 320, 8>;
constexpr int DEGMAX = 8;          // lines per bus
constexpr int BINJMAX = 8;         // injections per bus

// l_info: from | to<<8 | flags<<24   (internal bus numbers = elimination positions)
constexpr uint32_t LF_EXISTS = 1u, LF_OWNER = 2u, LF_LIMITED = 4u;
// i_info: bus | kind<<8
constexpr uint32_t IK_NONE = 0u, IK_REAL = 1u, IK_VIRTUAL = 2u;

// Static solver schedule.  Passes [0, npass_upd) are PK_UPD, then npass_inv PK_INV, then PK_BWD.
// The last npass_updq PK_UPD passes hold at most RW / 4 tasks each (the top of the elimination tree) and come in QUARTER form: four lanes
// per task, lane 2r + c updating the single element T[r][c] -= (Wa[r] * inv(D)) . Wb[c] -- the same arithmetic per element, six LDS
// instructions per pass instead of ten, which is what a pass costs whatever its fill.  Quarter descriptor = (&T[r][c], &Wa[r][0], &Wb[c][0], D).
// In front of them, npass_updh passes of at most RW / 2 tasks in HALF form: two lanes per task, lane r updating the row T[r][:] (seven LDS
// instructions).  Half descriptor = (&T[r][0], &Wa[r][0], Wb, D).
//   PK_UPD  T -= Wa * inv(D) * Wb'         task = (T, Wa, Wb, D)      BYTE offsets into W of 2x2 blocks (bit 15 of T = rhs task; full form only)
//   PK_INV  P = inv(D); y <- P * y         task = (D, Y, P, -)
//   PK_BWD  y_i -= P_i * W' * x_a          task = (Y_i, W, P_i, Y_a)
//           half form (a pass of at most RW / 2 tasks): two lanes per task, lane r updating y_i[r] -= P_i[r][:] . (W' x_a) -- six LDS instructions
//           instead of seven.  Half descriptor = (&Y_i[r], W, &P_i[r][0], Y_a).
//
// Per-scenario solver workspace W (doubles), 2x2 blocks row-major [tt, tl, lt, ll]:
//   [0, 4*nb)                 diagonal blocks  D_i = [[M_ii, B_ii], [B_ii, -E_i]]
//   [4*nb, 4*(nb+noff))       off-diagonal blocks K(a, i), a eliminated after i (lines and fill)
//   [off_rhs, off_rhs+4*nb)   right-hand side as a pseudo-bus: block i = [[y_theta, y_lambda], [0, 0]]
//   [off_p, off_p+4*nb)       P_i = inv(D_i) after the factorisation
//
// Idle lanes.  A lane without a task in a pass does not hold a null descriptor in the device image: it SHADOWS an active lane of the pass
// (the same read operands, so its loads are broadcasts of addresses the pass reads anyway) and carries an idle marker the kernel tests with
// one compare.  A kernel instantiation may then run the loads and the arithmetic of a pass on all lanes and predicate only the stores.
//   PK_UPD (all forms), PK_BWD (both forms): field 0 == field 3.  No real task has it: an update's target T is an off-diagonal block, the
//           diagonal block of a bus eliminated LATER than the pivot's, or an rhs pair (bit 15 set in the full form) -- never the pivot block D
//           itself; a back substitution's y_i and y_a belong to different buses (i < a).  The idle lane reads the pivot block as its target.
//   PK_INV: fields 2 and 3 non-zero (TASK_IDLE_INV); a real inversion task leaves them zero.
// case_symbolic asserts both when it builds the image.  Descriptors behind the last pass (the one-pass-ahead prefetch reads one) stay 0xffff.
constexpr uint16_t TASK_IDLE_INV = 0xffff;
inline bool task_idle(const uint16_t* t, bool inv) { return inv ? (t[2] | t[3]) != 0 : t[0] == t[3]; }

template <class TL>
struct DevCaseT {
    static constexpr int NBT = TL::NBT, NLT = TL::NLT, NIT = TL::NIT, NCOMPMAX = TL::NCOMPMAX, MAXPASS = TL::MAXPASS, MAXOFF = TL::MAXOFF, ROWL = TL::RW;
    int32_t nb, ng, nl, nd, ninj, ncomp, ref_bus, noff;
    double base_mva, total_load;
    uint32_t exist_mask;            // bit i = bus i exists (16-lane tile only)
    uint32_t nws;                   // doubles in W
    uint16_t off_rhs, off_p;
    uint16_t npass, npass_upd, npass_inv, nzero;
    uint16_t maxdeg, maxinj, base_connected, npass_updq;   // npass_updq: the last PK_UPD passes in quarter form (below)   // base_connected: the network with every line in service is one island   // largest number of lines / injections at one bus
    uint16_t maxdeg_s[2], maxinj_s[2];   // longest line / injection list among the buses of bus slot 0 / 1
    uint16_t npass_updh, pad3[3];   // PK_UPD passes in half form, in front of the quarter-form ones
    uint64_t bwd_half;              // bit k: PK_BWD pass k (counted from the first one) is in half form; all of them or none (relmc_case_load)
    uint64_t b_line8[NBT];          // the bus' line list packed one byte each (id | 0x80 = 'to' end), unused entries = nl (the all-zero record)
    uint64_t b_inj8[NBT];           // the bus' injection list packed one byte each, unused entries = ninj (the all-zero record)
    // lines
    double b_bsum[NBT];             // sum of the susceptances of the bus' lines, in list order (all lines in service)
    double l_b[NLT];
    double l_rate[NLT];             // p.u. (0 = unlimited)
    uint32_t l_info[NLT];
    int32_t l_partner[NLT];         // the other line of the same bus pair, -1 if none
    uint16_t l_blk[NLT];            // owner lines: W offset of the pair's off-diagonal block
    // injections (real generators then virtual generators = loads)
    // per injection {upper bound p.u., lower bound p.u., cost c1 * baseMVA (opf_setup), original Pmin in MW (nodal shed = Pg - Pmin,
    // mc_simulation.m:86)}: bounds and cost come in with one or two 16-byte LDS reads
    alignas(16) double i_tab[NIT][4];
    uint32_t i_info[NIT];
    // per-bus incidence
    uint8_t b_nline[NBT];
    uint8_t b_line[NBT][DEGMAX];    // line id | 0x80 when the bus is the line's 'to' end
    uint8_t b_ninj[NBT];
    uint8_t b_inj[NBT][BINJMAX];
    int16_t b_vinj[NBT];            // virtual generator at the bus, -1 if none
    uint8_t b_ext[NBT];             // internal bus -> external bus number
    uint8_t b_lane[NBT];            // bus held by lane r of bus slot t at [RW * t + r] (0xff = none): the partly filled last slot gets the buses with the
                                    // shortest incidence lists, because a slot's gather loops run to the longest list among its buses (relmc_case_load)
    uint8_t b_int[NBT];             // external bus number -> internal bus
    uint32_t thr[NCOMPMAX];         // Bernoulli thresholds floor(U*2^32)
    // static schedule of the sparse block LDL' (computed once per case on the host)
    uint16_t zero_off[MAXOFF];      // W offsets of fill-only blocks (cleared every iteration)
    uint8_t pass_ntask[MAXPASS];
    uint16_t task[MAXPASS][ROWL][4];    // byte offsets into the scenario's workspace (< 32 KiB); a lane without a task shadows an active one and carries the idle marker (above)
    // Fill blocks cleared by the spare lanes of the assembly's block stores (relmc_schedule.hip: fill_lanes; read only by an instantiation with
    // kFillBySlot, relmc_kernels.hip).  A lane of a line slot that holds no owner line, and a lane of a bus slot that holds no bus, stores exact
    // zeros with the block stores its slot issues anyway; given the W offset of a fill block it clears that block.  zero_off's entries
    // [nzero_res, nzero) are assigned, nfill_line of them to line-slot lanes and nfill_bus to bus-slot lanes; [0, nzero_res) found no spare lane
    // and keep the loop.  The tables stand behind the pass schedule, outside the part every workgroup copies to LDS: every field
    // above keeps its offset and the LDS image its size.
    uint16_t l_blk_fill[NLT];       // l_blk with the spare lanes' fill blocks filled in; 0xffff = the lane of line slot s at [RW * s + r] stores no block
    uint16_t b_lane_fill[NBT];      // b_lane with the spare lanes carrying the POSITION of a fill block (W offset / 4, >= nb); 0xffff = none
    uint16_t nzero_res, nfill_line, nfill_bus;
    uint16_t nidle_line, nidle_bus_s[2];   // lanes of the line slots / of bus slot 0, 1 that store no block at all (0: the slot's block stores need no predicate)
    uint16_t pad4[2];
};

// per-lane partial accumulators written once per workgroup-row, reduced by relmc_finalize_kernel
template <class TL>
struct PartialT {
    double dns, dns2;
    double shed[TL::IS];
    uint32_t n, nfail, nsing, ninf, nnc, iters;
    uint32_t cf_inj[TL::IS];
    uint32_t cf_line[TL::LS];
    uint32_t pad;
};

// Dynamic tail of the fused path on the 16-lane tile (relmc_eval_kernel, phase B): the fp64 contributions of one claimed scenario group,
// parked until relmc_tail_replay_kernel adds them to the record of the wavefront that owns the group.  Item p = k * W + owner is tail group
// k of wavefront `owner` (W wavefronts in the grid).  flag[row] is written by every claim; dns[row] and the row's lanes' shed[] only with flag 1.
template <class TL>
struct TailRecT {
    double shed[64][TL::IS];        // per lane of the wavefront
    double dns[TL::SPW];            // per scenario row
    uint32_t flag[TL::SPW];         // per scenario row: 1 = the static assignment adds this row's dns (and its non-zero shed[])
};

// one unit the primary schedule did not converge on
struct FailRec {
    unsigned long long unit;        // launch-local index + unit_base: sample offset (MODE 0), state (1), year * hours + hour (2), distinct state (3), row offset (4)
    uint32_t weight, pad;
    uint32_t mask[8];               // outage mask words
};

struct EvalArgs {
    uint64_t seed, first_index;
    int64_t n;
    // solver options
    int32_t policy, max_it;
    double feastol, gradtol, comptol, costtol, xi, sigma, z0, alpha_min, max_stepsize;
    // explicit states in / per-scenario results out (materialised mode), device pointers
    const uint8_t* states;
    double* dns;
    double* nodal;
    int32_t* status;
    int32_t* iters;
    void* partial;                  // PartialT<tile>[gridDim.x * blockDim.x]
    uint32_t prio_mode;             // issue-priority balancing between co-resident wavefronts: 0 off, 1 by grid half, 2 by wave half
    uint32_t scen_doubles;          // per-scenario LDS doubles (workspace + stash), = 2 mod 4
    uint32_t stash_off;             // start of the per-lane stash behind the workspace
    uint32_t case_bytes;            // bytes of the case tables copied to LDS (everything before the pass schedule)
    unsigned long long* timing;     // profiling builds: [waves][8] phase cycle counters (else null)
    double fail_threshold;          // loss flag: dns > 1e-4 (nsqMain.m:270) / > 0.01 (seqMain.m:41)
    const double* load_scale;       // MODE 1: optional per-scenario load scale factor
    // MODE 2 (sequential): chronology masks [years][hours][OW x u32], compacted contingency hours, hourly load curve
    const uint32_t* seq_masks;
    const uint32_t* seq_offsets;    // [years + 1] exclusive scan of contingency-hour counts
    const uint16_t* seq_hours;      // [years][hours] contingency hours of each year, ascending
    const double* load_factors;     // [hours]
    double* curt;                   // [years][hours] hourly curtailment (MW), zero where not evaluated
    int32_t seq_nyears, seq_hpy;
    // MODE 3 (distinct states with multiplicities, nsqMain.m:220-245): scenario u = state memo_keys[memo_perm[memo_start[u]]]
    // counted memo_start[u+1] - memo_start[u] times
    const uint32_t* memo_keys;      // [n][OW] outage masks of the sampled range
    const uint32_t* memo_perm;      // [n] sample indices sorted by mask
    const uint32_t* memo_start;     // [n_distinct + 1] first sorted position of every distinct mask
    // MODE 4 (rows of the persistent state database): scenario u = row db_first + u, key words at memo_keys[row][OW],
    // results go to dns[row], status[row] (packed) and nodal[row][nb].  Behind the zero-curtailment pre-screen memo_perm lists the new rows the
    // certificate did not cover: scenario u = row db_first + memo_perm[u] (null = all rows)
    // MODE 7 (fused path behind the pre-screen): scenario u = sample memo_perm[u] of the range, state memo_keys[memo_perm[u]][OW]
    int64_t db_first;
    // Units (samples / states / rows) that end non-converged (status 1 or 2) are listed here instead of being accumulated; the host
    // evaluates them again under further elimination orders (relmc_retry.hip: fail_retry).  Null = off.
    uint32_t* fail_count;
    FailRec* fail_list;
    uint32_t fail_cap;
    int32_t tail_groups;            // dynamic tail (below), 0 = static assignment
    int64_t unit_base;              // added to the launch-local unit index (chunked host-buffer pipeline)
    // MODE 6 (dense pivoted last resort): [scenario rows of the grid][dense_stride] doubles of global scratch, dense_stride >= 2 nb (2 nb + 1)
    // Dynamic tail (MODE 0 on the 16-lane tile; TailPlan in relmc_ctx.h): the last tail_groups groups of every wavefront's range are handed out
    // through *tail_count (zero at launch), their fp64 contributions parked in tail_rec = TailRecT<tile>[wavefronts * tail_groups].  The two
    // pointers share their words with MODE 6's, which no MODE 0 launch uses: the argument block keeps its size and every field its offset.
    union { double* dense; void* tail_rec; };
    union { uint64_t dense_stride; uint32_t* tail_count; };
    uint32_t norms_always;          // diagnosis: every trip of the interior-point loop accumulates the second-stage termination norms (kNormSplitMask)
};

// Zero-curtailment certificate (relmc_screen.hip; SURVEY 8f rank 4, mc_simulation.m:57-59, 65): tables built by relmc_case_load on the host, resident in
// HBM, read through the vector-memory path.  A state is certified when the units in service, loaded proportionally between Pmin and Pmax,
// serve the whole load with every DC flow inside (or on) its rating: base-topology PTDF, one or two lines out through the outage system
// (I - H_MM) x = F_M, more lines out never.
struct ScreenTab {
    int32_t nl, ng, valid, pad;
    double total_load;              // MW at load scale 1
    double sum_pmin, sum_rng;       // MW over all units: sum Pmin, sum (Pmax - Pmin)
    const double* pmin;             // [ng] MW
    const double* rng;              // [ng] MW, Pmax - Pmin
    const double* f_min;            // [nl] MW flow of (all units at Pmin) through the PTDF
    const double* f_rng;            // [nl] MW flow of (all units' ranges)
    const double* f_load;           // [nl] MW flow of the bus loads at scale 1 (positive = the loads' own contribution, subtracted)
    const double* lim;              // [nl] MW rating + 1e-9 MW of rounding slack; +inf = no limit
    const double* gpair;            // [nl][ng][2] {PTDF[l, bus(k)] * Pmin_k, PTDF[l, bus(k)] * (Pmax_k - Pmin_k)}, 16-byte aligned pairs
    const double* hmat;             // [nl (line out m)][nl] H[m][l]: flow on l per MW sent from from(m) to to(m) in the base topology (the outage formulas' matrix)
    const uint8_t* bridge;          // [nl] 1 = taking the line out splits the network (1 - H[m][m] = 0; the certificate tests that itself)
};

// device image of relmc_acc (include/relmc.h): 6 + 256 + 1 int64, then 2 + 128 doubles
struct DevAcc {
    long long n, n_fail, n_singular, n_infeasible, n_nonconverged, sum_iters;
    long long comp_fail[256];
    long long n_screened;           // never written by the evaluation kernels: the pre-screen's count is added on the host (relmc_screen.hip)
    double sum_dns, sum_dns2;
    double sum_nodal[128];
};

constexpr int FIN_ITEMS = 8 + 256 + 128;

constexpr int NCOMPMAX = 128;       // unit capacity of the HL1 fleet tables
constexpr int SEQ_NCOMPMAX = 256;   // component capacity of the sequential chronology (both tiles)
struct SeqCase {
    int32_t ncomp, hpy, mw, pad;    // mw: 32-bit mask words per hour (= the tile's OW: 4 or 8)
    double mttf[SEQ_NCOMPMAX], mttr[SEQ_NCOMPMAX];
};

struct Hl1Case {
    int32_t ngen, nhours;
    uint32_t thr[NCOMPMAX];          // unit g down iff draw < thr[g]  (up iff rand() >= for_rate)
    double cap[NCOMPMAX];
};

// HL1 sequential chronology (relmc_hl1_seq): the fleet's rates and the stationary start thresholds, mirrored by include/relmc.h's contract
struct Hl1SeqCase {
    int32_t ngen, nhours;
    double cap[NCOMPMAX], mttf[NCOMPMAX], mttr[NCOMPMAX];
    double q[NCOMPMAX];              // mttr / (mttf + mttr): RELMC_HL1_START_STATIONARY starts unit k DOWN iff draw 0 < q[k]
};
constexpr int HL1_SEQ_WINDOW = 512;  // hours per LDS window of relmc_hl1_seq_kernel (a wavefront's masks: WINDOW x 4 x u32 = 8 KB)
// HL1 sequential chronology with three-state units (relmc_hl1_ms_seq): per unit the capacities of UP and DERATED, per state the mean
// holding time and the probability of the first-listed destination, and the stationary start thresholds, as include/relmc.h's contract
struct Hl1MsCase {
    int32_t ngen, nhours;
    double cap[NCOMPMAX][2];         // capacity_mw, derated_mw
    double mean[3][NCOMPMAX], first_p[3][NCOMPMAX];
    double thr_down[NCOMPMAX];       // pi_2: RELMC_HL1_START_STATIONARY starts unit k DOWN iff draw 0 < thr_down[k],
    double thr_out[NCOMPMAX];        // pi_2 + pi_1: else DERATED iff draw 0 < thr_out[k], else UP
};
constexpr int HL1_MS_WINDOW = 256;   // hours per LDS window of relmc_hl1_ms_kernel (a wavefront's two planes: 2 x WINDOW x 4 x u32 = 8 KB)
// Loss events of the HL1 sequential chronology (relmc_hl1_seq_events) in summary: one chain's, or one reduction slice's.  The integer
// fields add exactly, the maxima combine by max.
struct Hl1EventRec {
    long long events, sum_dur, sum_dur2, max_dur, censored;
    double sum_energy, sum_energy2, max_energy, max_peak;
};
// Loss events of the sequential HL2 track (relmc_seq_events) in summary: one reduction slice's.  Integers add, maxima combine by max.
struct SeqEventPart {
    long long events, censored, load_onset, sum_dur, sum_dur2, max_dur;
    double sum_energy, sum_energy2, max_energy, max_peak;
};
constexpr int SEQ_EVENT_MW = SEQ_NCOMPMAX / 32;   // mask words of an event record (relmc_seq_event::onset / involved)
// the per-component arrays of relmc_seq_event_acc, in its order (copied to its tail as they stand)
struct SeqEventComp {
    long long onset_events[SEQ_NCOMPMAX], involved_events[SEQ_NCOMPMAX];
    double onset_energy[SEQ_NCOMPMAX], involved_energy[SEQ_NCOMPMAX];
};

// HL1 planning model (relmc_hl1_plan): maintenance windows, ELU slots and Bernoulli thresholds, mirrored by include/relmc.h's contract
constexpr int PLAN_MAX_ELU = 8;
constexpr uint32_t PLAN_TAG = 0x20000000u;

// one unit, 32 bytes: a single scalar load per unit and hour
struct __attribute__((aligned(32))) PlanUnit {
    double cap;
    uint32_t thr;                    // down iff its word < thr
    int32_t slot;                    // ELU slot 0..7 (unit order), -1 = not energy-limited
    int32_t mlo, mhi;                // in maintenance at hour h iff mlo <= h < mhi (0-based hours, clipped to the year; mlo = mhi = 0: none)
    int32_t pad[2];
};

struct PlanCase {
    int32_t ngen, nhours, n_elu, nblk;   // nblk = Philox blocks per hour = (ngen + 5) / 4 (words 0, 1: LFU normal; word 2 + k: unit k)
    double sigma;                        // LFU standard deviation, MW
    double elu_cap[PLAN_MAX_ELU], elu_lim[PLAN_MAX_ELU];   // unused slots: capacity 0, limit +inf
    PlanUnit unit[NCOMPMAX];
};

// HL1 multi-area chronology (relmc_hl1_area): the relmc_hl1_seq fleet stored area-major, each area's unit range and the tie topology,
// mirrored by include/relmc.h's contract (AREA_MAX = RELMC_AREA_MAX)
constexpr int AREA_MAX = 8;
constexpr int AREA_MAX_AUG = 4096;   // augmenting paths per step at most (a guard: Edmonds-Karp on 8 areas needs far fewer)
struct AreaCase {
    int32_t ngen, nhours, n_areas, pad;
    int32_t lo[AREA_MAX + 1];        // area a owns units [lo[a], lo[a + 1]); lo[n_areas] = ngen
    double cap[NCOMPMAX], mttf[NCOMPMAX], mttr[NCOMPMAX];
    double q[NCOMPMAX];              // mttr / (mttf + mttr), as Hl1SeqCase
    double tie[AREA_MAX * AREA_MAX]; // T[i][j] at i * n_areas + j: summed tie capacities, symmetric, zero diagonal
};
// The ties one by one, for relmc_hl1_area_tie_outages (AREA_TIE_MAX = RELMC_HL1_TIE_MAX: one mask word; AREA_TIE_DRAW_BASE =
// RELMC_HL1_TIE_DRAW_BASE: tie t draws as component 128 + t).  mttf = +inf: the tie never fails (mttr and q unused, stored as 1 and 0).
constexpr int AREA_TIE_MAX = 32;
constexpr int AREA_TIE_DRAW_BASE = 128;
struct AreaTies {
    int32_t n_ties, pad;
    int32_t from[AREA_TIE_MAX], to[AREA_TIE_MAX];            // 0-based areas
    double cap[AREA_TIE_MAX], mttf[AREA_TIE_MAX], mttr[AREA_TIE_MAX];
    double q[AREA_TIE_MAX];                                  // mttr / (mttf + mttr)
};
// The levels of relmc_hl1_area_sweep as the kernel reads them (AREA_SWEEP_MAX_LEVELS = RELMC_HL1_AREA_SWEEP_MAX_LEVELS), prepared by the
// host: 7.2 KB at 8 levels, beyond the 4 KB kernel-argument segment, so the table lives in a device buffer of the context and every read
// of it is a scalar load at a wave-uniform address.
constexpr int AREA_SWEEP_MAX_LEVELS = 8;
struct AreaSweepLevelTab {
    double scale[AREA_MAX], shift[AREA_MAX];                 // load of area a: scale[a] * load[a][h] + shift[a]
    double tie[AREA_MAX * AREA_MAX];                         // the level's T with every tie UP, formed as relmc_hl1_area_load forms AreaCase::tie
    double cap[AREA_TIE_MAX];                                // the level's capacity of tie t (read with outage data only)
};
struct AreaSweepTab {
    AreaSweepLevelTab lv[AREA_SWEEP_MAX_LEVELS];
    uint32_t withheld[4];                                    // bit k & 31 of word k >> 5: global unit k is not part of fleet 1
    int32_t n_levels;
    uint32_t fleet1;                                         // bit j: level j uses fleet 1
    uint32_t solve;                                          // bit j: a tie of level j has a capacity > 0 (else T is all zero in every step)
    int32_t pad;
};

}  // namespace relmc
