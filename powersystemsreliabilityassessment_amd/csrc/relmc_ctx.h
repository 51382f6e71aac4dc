// relmc_ctx.h — what the translation units of librelmc.so share: the context behind the opaque relmc_ctx handle of include/relmc.h, the
// error helpers, and the internal entry points each unit offers the others.  Host code only orchestrates (case tables -> HBM, launches on
// the context's stream, HIP-event timing, deterministic partial reduction on the device, estimator arithmetic); there is no CPU
// evaluation path anywhere in the library.
//
//   relmc_schedule.hip   symbolic analysis of a case and the static solver schedule (host arithmetic only), the order tuner
//   relmc_core.hip       context lifetime, relmc_case_load + order calibration, the evaluation-kernel launcher, mc_sampling, estimators
//   relmc_retry.hip      units the primary elimination order does not converge on: further static orders, dense pivoted last resort
//   relmc_simulate.hip   mc_simulation (host-buffer pipeline), the fused nsq_accumulate
//   relmc_nsq_run.hip    the nsqMain loop for any number of ranks (relmc_nsq_run) and its stretch-length rule
//   relmc_database.hip   the reference's dedupe and persistent unique-state database on the device
//   relmc_comm.hip       the path's single collective: RCCL (bound at run time) or a host-supplied all-reduce, with a wall-clock guard
//   relmc_seq.hip        sequential track (chronology, scaled-load hours, annual indices, the seqMain loop), the HL1 copper sheet, the HL1
//                        sequential chronology (relmc_hl1_seq), its loss events (relmc_hl1_seq_events) and its load sweep
//                        (relmc_hl1_seq_sweep), three instantiations of the one kernel template of relmc_hl1_chain_kernels.h, and
//                        the record reduction and unit check of every HL1 chronology track
//   relmc_hl1_host.h     (a header, included by the eleven HL1 units around it) what their host code shares: the chunk rule, the loop over a
//                        model's launches with the reduction of their year records (hl1_run_records), the argument and unit checks, and the one
//                        copy of what the storage and weather-year tracks check and fill alike (storage fields, resource scales, pick,
//                        weather_host, the two-row copies, relmc_hl1_storage_acc)
//   relmc_hl1_storage_devfn.h (a header, no kernel) the device leaves those four tracks share: the storage step, its bits, the year close,
//                        the weather pick
//   relmc_storage.hip    energy storage with a state of charge on that chronology (relmc_hl1_seq_storage, kernel in relmc_hl1_storage_kernels.h)
//   relmc_variable.hip   weather-year wind and solar resources on that chronology, with those storages (relmc_hl1_var_load, relmc_hl1_var_seq,
//                        kernel in relmc_hl1_storage_kernels.h)
//   relmc_stress.hip     weather-dependent forced outage rates on that chronology, with those resources and storages (relmc_hl1_stress_load,
//                        relmc_hl1_stress_seq, kernel in relmc_hl1_storage_kernels.h)
//   relmc_maint.hip      planned maintenance on that chronology, up to 8 schedules on one fleet history (relmc_hl1_maint_load,
//                        relmc_hl1_maint_seq; the kernel is the fourth model of relmc_hl1_chain_kernels.h's template)
//   relmc_attr.hip       loss attribution on that chronology: every loss step charged to the units that are down (relmc_hl1_attr_seq,
//                        kernels in relmc_hl1_attr_kernels.h)
//   relmc_multistate.hip that chronology with three-state units (relmc_hl1_ms_load, relmc_hl1_ms_seq, kernel in relmc_multistate_kernels.h)
//   relmc_plan.hip       the HL1 planning model's Monte Carlo (relmc_hl1_plan)
//   relmc_area.hip       the HL1 multi-area chronology with tie-line transfers (relmc_hl1_area)
//   relmc_area_sweep.hip the sweep of that chronology over load, tie and fleet levels (relmc_hl1_area_sweep, kernel in relmc_area_sweep_kernels.h)
//   relmc_area_variable.hip weather-year resources and storages in the areas of that chronology (relmc_hl1_area_var_load, relmc_hl1_area_var,
//                        kernel in relmc_area_kernels.h, its own leaves in relmc_area_variable_devfn.h)
//   relmc_screen.hip     the zero-curtailment pre-screen (relmc_solver_opts.screen): certificate tables, pre-pass kernels, worklists
//   relmc_importance.hip importance sampling for the non-sequential track: tilted sampler with likelihood ratios, weighted reductions (kernels in
//                        relmc_is_kernels.h), the cross-entropy tuner and the weighted run loop
//   relmc_debug.hip      introspection and test hooks that are not part of include/relmc.h
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/relmc.h"
#include "relmc_dev.h"

// Diagnosis switches of a context.  The default build sets them through relmc_debug_set only (tests); a -DRELMC_DEV_SWITCHES build
// (csrc/Makefile: ablate/librelmc_dev.so) also reads the RELMC_* environment variables of the same names once at relmc_ctx_create.
struct relmc_switches {
    bool no_retry = false;           // the first attempt's results as they are (no list of non-converged units)
    bool retry_dense_first = false;  // listed units straight to the dense pivoted solve
    bool nsq_no_stretch = false;     // relmc_nsq_run: one launch per batch
    bool db_no_probe = false;        // state database: every batch through the dedupe, no per-sample probe
    bool dynamic_shape = false;      // fused path: the run-time-shape evaluation kernel even when the case has the compiled-in shape
    bool static_tail = false;        // fused path on the 16-lane tile: no dynamic tail (T = 0), every group run by the wavefront that owns it
    bool norms_always = false;       // evaluation kernels: the second-stage termination norms on every trip, not only on the trips that can end
};

namespace relmc_host {
// Owner of n elements of T in device memory (hipMalloc) or pinned host memory (hipHostMalloc); move-only, released by the destructor.
// grow(n) discards: a buffer smaller than n is released and n elements are allocated, contents not kept; on failure it is left empty.
// The release is a plain hipFree / hipHostFree, which waits for the device: a buffer may be dropped while a queued kernel still reads it.
template <class T, bool Pinned = false>
class Buffer {
public:
    Buffer() = default;
    Buffer(Buffer&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
    Buffer& operator=(Buffer&& o) noexcept
    {
        if (this != &o) { reset(); p_ = o.p_; n_ = o.n_; o.p_ = nullptr; o.n_ = 0; }
        return *this;
    }
    ~Buffer() { reset(); }
    T* get() const { return p_; }
    size_t size() const { return n_; }
    void reset()
    {
        if (p_) (void)(Pinned ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr; n_ = 0;
    }
    hipError_t grow(size_t n)
    {
        if (n <= n_) return hipSuccess;
        reset();
        void* p = nullptr;
        const hipError_t e = Pinned ? hipHostMalloc(&p, sizeof(T) * n, hipHostMallocDefault) : hipMalloc(&p, sizeof(T) * n);
        if (e == hipSuccess) { p_ = static_cast<T*>(p); n_ = n; }
        return e;
    }
private:
    T* p_ = nullptr;
    size_t n_ = 0;
};
template <class T> using DevBuf = Buffer<T, false>;
template <class T> using PinBuf = Buffer<T, true>;
// The device buffers of an HL1 record model (relmc_hl1_host.h, hl1_run_records): the year records of one launch and the block partials of
// their reduction, grow-only.  Every model keeps a pair of its own.
struct Hl1Records { DevBuf<double> years, part; };
}  // namespace relmc_host

struct relmc_ctx {
    template <class T> using DevBuf = relmc_host::DevBuf<T>;
    template <class T> using PinBuf = relmc_host::PinBuf<T>;
    using Hl1Records = relmc_host::Hl1Records;
    static constexpr size_t kCaseBytes = sizeof(relmc::DevCaseT<relmc::Tile96>) > sizeof(relmc::DevCaseT<relmc::Tile24>) ? sizeof(relmc::DevCaseT<relmc::Tile96>)
                                                                                                                      : sizeof(relmc::DevCaseT<relmc::Tile24>);
    int device = -1;
    relmc_switches sw;
    // relmc_seq_years' device buffers, kept between calls (six hipMalloc / hipFree pairs per call were 1 ms of a 17 ms step): grow-only
    struct SeqStep {
        DevBuf<uint32_t> dm, counts, off;    // counts: [0, n) listed hours per year, [n, 2 n) contingency hours per year (pre-screen)
        DevBuf<uint16_t> hours; DevBuf<double> curt, year;
    } sq;
    // loss events of that step (relmc_seq_events; relmc_debug_seq_events on caller-given hours): grow-only year counts / list offsets, the
    // list, reduction partials, histogram, per-component arrays
    struct SeqEvents {
        DevBuf<long long> count, offset; DevBuf<relmc_seq_event> list; DevBuf<relmc::SeqEventPart> part; DevBuf<unsigned long long> hist;
        DevBuf<relmc::SeqEventComp> comp;
    } sq_events;
    std::vector<int32_t> order_hint;     // relmc_case_order_hint: primary elimination order of the next relmc_case_load (external bus numbers), empty = the rule
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool has_case = false;
    int tile = 0;                        // 0: Tile24 (16-lane rows), 1: Tile96 (one scenario per wavefront)
    relmc::DevCaseT<relmc::Tile24> hcase24;
    relmc::DevCaseT<relmc::Tile96> hcase96;
    DevBuf<uint8_t> dcase;               // device image of the active tile's case (kCaseBytes)
    int nb = 0, ng = 0, nl = 0, ncomp = 0;
    DevBuf<uint8_t> dpartial;
    DevBuf<uint8_t> dtail;               // TailRecT<Tile24>[wavefronts * T] of the fused path's dynamic tail, allocated at the first launch that has one
    int last_tail_groups = 0; int64_t tail_launches = 0;   // T of the last fused launch on the 16-lane tile, launches with T > 0 so far (relmc_debug_tail_groups)
    DevBuf<relmc::DevAcc> dacc;
    struct HostStage { relmc_acc acc; uint32_t fail_cnt, pad; };
    PinBuf<HostStage> hstage;            // accumulators + listed-unit count of a first-attempt launch come back in one synchronisation (eval_collect)
    int num_cu = 0;
    int blocks_per_cu = 0;
    uint32_t scen_doubles = 0, lds_bytes = 0, stash_off = 0;
    bool shape_static = false;           // the primary image has the compiled-in shape (relmc_shape_rts24.h): MODE 0 launches use that instantiation
    DevBuf<unsigned long long> dtiming; int timing_waves = 0;
    struct History { DevBuf<double> d; PinBuf<double> h; } hist;      // per-sample dns of one launch (checkpoint histories of small batches, relmc_nsq_run)
    // distinct-state path: device buffers sized for the samples of a dedupe
    struct Memo {
        DevBuf<uint32_t> k, perm0, perm1, head, uid, start, nu;
        DevBuf<unsigned long long> ch0, ch1; DevBuf<uint8_t> tmp;
        DevBuf<uint32_t> miss, k2;           // probe-first database path: miss list (sample indices) and the masks of the misses
    } memo;
    // persistent state database (nsqMain.m:91-99): rows in HBM, open-addressing table of row ids
    struct Database {
        int64_t cap = 0, n = 0, samples = 0;     // cap: rows the five row arrays hold (the table has at least twice as many slots)
        DevBuf<uint32_t> keys; DevBuf<unsigned long long> count; DevBuf<double> dns; DevBuf<int32_t> meta; DevBuf<double> nodal; DevBuf<uint32_t> table;
        DevBuf<relmc::DevAcc> partial;
        DevBuf<unsigned long long> snap;         // row counts before a stretch of small batches (relmc_nsq_run)
        bool has_opts = false; relmc_solver_opts opts = {};
        bool invalid = false;                    // an entry point failed between the count bumps of a batch and its bookkeeping: relmc_db_reset / relmc_case_load only
    } db;
    // retry of the units the primary elimination order does not converge on: a second device image of the case built with
    // another static order (lazily, from a copy of the description), the kernel's list of such units, scratch rows for their re-evaluation
    struct CaseCopy {
        relmc_case_desc d; bool valid = false;
        std::vector<double> bus_pd, inj_pmin, inj_pmax, inj_cost, br_b, br_rate, unavail; std::vector<int32_t> inj_bus, br_from, br_to; std::vector<uint8_t> always_up;
    } case_copy;
    static constexpr int kAlt = 2;           // further static orders: [0] the primary rule with the ties broken the other way, [1] fill first
    int alt_state[kAlt] = {0, 0};            // 0 not built yet, 1 ready, -1 unavailable (that order does not fit the tile)
    DevBuf<uint8_t> dcase_alt[kAlt]; uint32_t alt_scen_doubles[kAlt] = {0, 0}, alt_lds_bytes[kAlt] = {0, 0}, alt_stash_off[kAlt] = {0, 0};
    struct Retry {
        // the kernel's list (grows with the size of the call, fail_arm).  fail_count holds kCountWords words: [0] the listed units, [1] the claim
        // counter of the dynamic tail, zero between launches (relmc_tail_replay_kernel puts it back); every clearing of the buffer clears both
        DevBuf<relmc::FailRec> fail; DevBuf<uint32_t> fail_count; bool fail_dirty = false;
        static constexpr size_t kCountWords = 2, kCountBytes = kCountWords * sizeof(uint32_t);
        DevBuf<double> dense;                // global scratch of the dense pivoted last resort (MODE 6)
        // scratch rows of the re-evaluation: twice `rows` listed units (the third order's compact rows start at `rows`)
        DevBuf<uint32_t> keys; DevBuf<double> dns; DevBuf<int32_t> meta; DevBuf<double> nodal, scale; int64_t rows = 0;
    } retry;
    int64_t retry_dense_units = 0, retry_dense_converged = 0;    // units that went to it since the case was loaded
    int64_t retry_overflow = 0;              // units that did not fit the list and kept their first-attempt results (relmc_retry_overflow)
    std::vector<double> hlf;                 // host copy of the hourly load factors (load scale of a re-evaluated hour)
    int64_t retry_units = 0, retry_converged = 0;        // since the case was loaded
    int order_primary = 0; int32_t order_probe[3] = {-1, -1, -1};   // which static order runs first, and the calibration's failure counts (-1 = not probed)
    // host-buffer entry points (relmc_mc_simulation, relmc_seq_mcsimulation): double-buffered chunk pipeline, device buffers
    // and pinned staging kept across calls
    struct HostPipe {
        bool ready = false; int ncomp = 0, nb = 0;
        hipStream_t up = nullptr, down = nullptr;
        hipEvent_t e_up[2] = {nullptr, nullptr}, e_ks[2] = {nullptr, nullptr}, e_ke[2] = {nullptr, nullptr}, e_down[2] = {nullptr, nullptr};
        struct Bufs {
            DevBuf<uint8_t> d_st; DevBuf<double> d_sc, d_dns, d_nod; DevBuf<int32_t> d_stat, d_it;
            PinBuf<uint8_t> h_st; PinBuf<double> h_sc, h_dns, h_nod; PinBuf<int32_t> h_stat, h_it;
        } buf[2];
    } pipe;
    // communicator over the ranks of a multi-GPU run (optional; relmc_comm_*): RCCL, or the host's own collective
    void* comm = nullptr; int comm_nranks = 0, comm_rank = -1;
    relmc_allreduce_fn host_allreduce = nullptr; void* host_allreduce_user = nullptr;
    relmc_allreduce_f64_fn host_allreduce_f64 = nullptr; void* host_allreduce_f64_user = nullptr;   // optional vector transport of the host collective
    int64_t comm_calls = 0; double comm_seconds = 0.0;                                     // all-reduces of relmc_acc through this context, wall time in them
    double comm_timeout_s = 120.0;                                                         // wall-clock guard of communicator init and of every collective
    void* watchdog = nullptr;                                                              // the guard's thread (relmc_comm.hip), started at the first guarded call
    DevBuf<double> dgather;                                                                // device staging of comm_allreduce_f64 (RCCL)
    // sequential track
    bool has_seq = false; relmc::SeqCase hseq; DevBuf<relmc::SeqCase> dseq; DevBuf<double> dlf;
    // HL1 copper-sheet model; lole / eue / part: relmc_hl1_nsq's device buffers, grow-only
    bool has_hl1 = false; int hl1_hours = 0;
    struct Hl1 { DevBuf<relmc::Hl1Case> dcase; DevBuf<double> sorted, suffix, lole, eue, part; } hl1;
    // HL1 sequential chronology (relmc_hl1_seq): its own fleet / load curve, the call's records
    bool has_hl1_seq = false;
    struct Hl1Seq { int ngen = 0, nhours = 0; DevBuf<relmc::Hl1SeqCase> dcase; DevBuf<double> load; Hl1Records rec; } hl1_seq;
    // loss events of that model (relmc_hl1_seq_events): grow-only chain records / counts / list offsets, reduction partials, histogram, list
    struct Hl1Events {
        DevBuf<relmc::Hl1EventRec> rec, part; DevBuf<long long> count, offset; DevBuf<unsigned long long> hist; DevBuf<relmc_hl1_event> list;
    } hl1_events;
    // load sweep on that model (relmc_hl1_seq_sweep): per-level records; storage on that model (relmc_hl1_seq_storage): records of both rows
    Hl1Records hl1_sweep, hl1_storage;
    // loss attribution on that model (relmc_hl1_attr_seq): year records, and grow-only the chains' unit records of one launch
    // unit[chain][ngen][4] with the partials of their reduction upart[slice][ngen][8]
    struct Hl1Attr { Hl1Records rec; DevBuf<double> unit, upart; } hl1_attr;
    // maintenance schedules of relmc_hl1_maint_load (relmc_hl1_maint_seq runs the fleet of hl1_seq under them): the mask table
    // tab[width][nhours][4] (bit k & 31 of word k >> 5 = unit k on maintenance; width = n_schedules rounded up to the kernel's 1, 2, 4 or 8,
    // the added schedules empty), the ngen and nhours it was built for, per-schedule records
    bool has_hl1_maint = false;
    struct Hl1Maint { int n_schedules = 0, ngen = 0, nhours = 0; DevBuf<uint32_t> tab; Hl1Records rec; } hl1_maint;
    // weather library of relmc_hl1_var_load (relmc_hl1_var_seq runs the fleet of hl1_seq against it): out[n_weather][n_res][nhours], the
    // optional load curves load[n_weather][nhours], records of both rows.  A slot of its own, apart from every other HL1 model
    bool has_hl1_var = false;
    struct Hl1Var { int n_weather = 0, n_res = 0, nhours = 0; bool has_load = false; DevBuf<double> out, load; Hl1Records rec; } hl1_var;
    // stress library of relmc_hl1_stress_load (relmc_hl1_stress_seq runs the fleet of hl1_seq against hl1_var's weather and it): the
    // cumulative multiplier tables cum[n_weather][n_classes][nhours + 1], the class of every unit, records of both rows.  A slot of its own
    bool has_hl1_stress = false;
    struct Hl1Stress { int n_weather = 0, n_classes = 0, nhours = 0, n_units = 0; DevBuf<double> cum; DevBuf<int32_t> ucls; Hl1Records rec; } hl1_stress;
    // HL1 sequential chronology with three-state units (relmc_hl1_ms_load / relmc_hl1_ms_seq): its own fleet / load curve, apart from every
    // other HL1 model; records of both rows
    bool has_hl1_ms = false;
    struct Hl1Ms { int ngen = 0, nhours = 0; DevBuf<relmc::Hl1MsCase> dcase; DevBuf<double> load; Hl1Records rec; } hl1_ms;
    // HL1 planning model (relmc_hl1_plan): its own fleet / maintenance / ELUs / load curve, per-year records, grow-only ELU energies and
    // hour loss counts
    bool has_hl1_plan = false;
    struct Hl1Plan { int nhours = 0, n_elu = 0; DevBuf<relmc::PlanCase> dcase; DevBuf<double> load, elu; Hl1Records rec; DevBuf<unsigned long long> hours; } hl1_plan;
    // HL1 multi-area chronology (relmc_hl1_area): its own areas / ties / load curves, per-row records
    bool has_hl1_area = false;
    // ties: the loaded ties one by one; tie_outages: relmc_hl1_area_tie_outages' data is in force (dties), tie_fail: with a finite mttf
    struct Hl1Area {
        int ngen = 0, nhours = 0, n_areas = 0; DevBuf<relmc::AreaCase> dcase; DevBuf<double> load; Hl1Records rec;
        std::vector<int32_t> tie_from, tie_to; std::vector<double> tie_cap;
        bool tie_outages = false, tie_fail = false; DevBuf<relmc::AreaTies> dties;
        // relmc_hl1_area_sweep (relmc_area_sweep.hip): the levels' table of a call, per-level, per-row records
        DevBuf<relmc::AreaSweepTab> sweep_tab; Hl1Records sweep_rec;
    } hl1_area;
    // weather library of relmc_hl1_area_var_load (relmc_hl1_area_var runs the areas of hl1_area against it): out[n_weather][n_res][nhours],
    // each resource's area, the optional load curves load[n_weather][n_areas][nhours], records of both kinds of every row.  A slot of its
    // own, apart from every other HL1 model
    bool has_hl1_area_var = false;
    struct Hl1AreaVar {
        int n_areas = 0, n_weather = 0, n_res = 0, nhours = 0; bool has_load = false; std::vector<int32_t> res_area;
        DevBuf<double> out, load; Hl1Records rec;
    } hl1_area_var;
    // zero-curtailment pre-screen (relmc_screen.hip): certificate tables of the case (device pointers inside tab), grow-only work buffers of a pre-pass
    struct Screen {
        relmc::ScreenTab tab = {};
        DevBuf<uint8_t> dtab;
        DevBuf<uint32_t> keys; DevBuf<uint8_t> flags; DevBuf<uint32_t> idx, dcount; DevBuf<uint8_t> tmp;
    } screen;
    hipEvent_t screen_ev0 = nullptr, screen_ev1 = nullptr;      // timing of the pre-pass
    // importance sampling (relmc_importance.hip): tilt tables of a call, grow-only per-sample buffers of one launch (at most 2^20 samples) and
    // reduction partials
    struct Is {
        DevBuf<uint32_t> thr; DevBuf<double> r_dn, r_up;
        DevBuf<uint8_t> states; DevBuf<double> w, dns, nodal, f_fail, f_dns, e; DevBuf<int32_t> status, iters;
        DevBuf<double> part_d, part_col; DevBuf<long long> part_i;
    } is;
    double last_kernel_ms = 0.0;
    long conflict_before = 0, conflict_after = 0;   // modelled extra LDS cycles per Newton step before / after the placement search
    long alt_conflict_before[kAlt] = {0, 0}, alt_conflict_after[kAlt] = {0, 0};      // the same of the further orders' images
    std::string err;
};

// The retry counters of a context at one moment.  A pass that is evaluated, cut and taken again over its used part (a stretch of relmc_nsq_run,
// a batch of relmc_seq_run) puts them back in between, so that relmc_retry_stats and its kin do not count the discarded pass.
struct RetryMark {
    int64_t units, converged, dense_units, dense_converged, overflow;
    explicit RetryMark(const relmc_ctx* c)
        : units(c->retry_units), converged(c->retry_converged), dense_units(c->retry_dense_units), dense_converged(c->retry_dense_converged), overflow(c->retry_overflow) {}
    void restore(relmc_ctx* c) const
    {
        c->retry_units = units; c->retry_converged = converged; c->retry_dense_units = dense_units; c->retry_dense_converged = dense_converged; c->retry_overflow = overflow;
    }
};

namespace relmc_host {

using namespace relmc;

extern const char* const kNoCtx;
int fail(relmc_ctx* ctx, int code, const std::string& msg);
bool verbose();                           // RELMC_VERBOSE in the environment (the library's only environment variable), read once
// index of the first NaN or infinite value of x[0, n), -1 if none (the input rule of the HL1 load calls, include/relmc.h)
inline int64_t first_non_finite(const double* x, int64_t n)
{
    for (int64_t i = 0; i < n; ++i)
        if (!std::isfinite(x[i])) return i;
    return -1;
}

#define HIP_TRY(ctx, expr)                                                                                   \
    do {                                                                                                     \
        hipError_t e_ = (expr);                                                                              \
        if (e_ != hipSuccess)                                                                                \
            return ::relmc_host::fail(ctx, RELMC_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

// ---- relmc_schedule.hip (no HIP call, no context) -----------------------------------------------------------------------------
struct SymOpts {
    const int32_t* order_hint = nullptr; int n_hint = 0;   // primary order from the host (external bus numbers, reference bus last); order_variant 0 only
    int place_moves = 100;               // moves per block of the LDS placement search (0: the order tuner's cost does not depend on the placement)
    long place_ww = 1;                   // weight of conflicts on operands that are written back
    bool no_quarter = false, no_half = false, no_bwd_half = false, no_bus_map = false;      // schedule forms off (ablation builds)
    int scen_pad4 = 0;                   // extra padding of a scenario row's LDS stride in units of 4 doubles (ablation builds)
    int model_leaf_free = -1;            // >= 0: scheduling MODEL with the pivots complete at assembly left out (relmc_debug_symbolic only: not a valid program)
};
struct SymGeom { uint32_t stash_off = 0, scen_doubles = 0, lds_bytes = 0; long conflict_before = 0, conflict_after = 0;
                 long shadow_masked = 0, shadow_tasks = 0, shadow_all = 0; };   // the same model on the finished device image: idle lanes masked / shadowing an active lane
SymOpts sym_opts_default();              // the shipped schedule; a RELMC_DEV_SWITCHES build reads the ablation variables here
template <class TL>
int case_symbolic(const relmc_case_desc* d, DevCaseT<TL>& C, int order_variant, const SymOpts& so, SymGeom& geom, std::string& err);
extern template int case_symbolic<Tile24>(const relmc_case_desc*, DevCaseT<Tile24>&, int, const SymOpts&, SymGeom&, std::string&);
extern template int case_symbolic<Tile96>(const relmc_case_desc*, DevCaseT<Tile96>&, int, const SymOpts&, SymGeom&, std::string&);
inline bool fits_tile24(const relmc_case_desc* d)
{
    return d->nb <= Tile24::NBT && d->nl <= Tile24::NLT && d->ng + d->nd <= Tile24::NIT && d->ng + d->nl <= Tile24::NCOMPMAX;
}
// The tile dispatch of the host code: fn(C) with a DevCaseT of the 16-lane tile or of the wide one on the heap; fn is generic in the tile
template <class F>
auto with_case_tile(bool tile24, F&& fn)
{
    if (tile24) { auto C = std::make_unique<DevCaseT<Tile24>>(); return fn(*C); }
    auto C = std::make_unique<DevCaseT<Tile96>>();
    return fn(*C);
}
// The device image of a case on the smallest tile that holds it: case_symbolic, then fn(image) -> code if that succeeded
template <class F>
int with_symbolic(const relmc_case_desc* d, int order_variant, const SymOpts& so, SymGeom& geom, std::string& err, F&& fn)
{
    return with_case_tile(fits_tile24(d), [&](auto& C) {
        const int rc = case_symbolic(d, C, order_variant, so, geom, err);
        return rc == RELMC_OK ? (int)fn(C) : rc;
    });
}

// ---- relmc_core.hip -----------------------------------------------------------------------------------------------------------
inline relmc_solver_opts solver_opts_or_default(const relmc_solver_opts* opts)
{
    relmc_solver_opts o;
    if (opts) o = *opts; else relmc_solver_opts_default(&o);
    return o;
}
inline bool screen_active(const relmc_ctx* ctx, const relmc_solver_opts& o) { return o.screen != 0 && ctx->screen.tab.valid != 0; }   // relmc_solver_opts.screen, and the case has its certificate tables
EvalArgs make_args(const relmc_solver_opts& o);
// launches relmc_eval_kernel<mode, active tile> on the context's stream between two events (default: ev0 / ev1); alt = 0 the primary image of
// the case, 1.. = the further orders'; *rows_out = scenario rows holding partial accumulators
int launch_eval(relmc_ctx* ctx, int mode, EvalArgs& a, int* rows_out, hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr, int alt = 0);
int launch_finalize(relmc_ctx* ctx, int rows);     // deterministic reduction of the partial records into ctx->dacc
int finish_timing(relmc_ctx* ctx);                 // stream synchronised, ctx->last_kernel_ms = ev0 .. ev1
int case_load_image(relmc_ctx* ctx, const relmc_case_desc* d, int order_variant);   // device image of the case under a further order (retry levels)
inline int mask_words(const relmc_ctx* ctx) { return ctx->tile == 0 ? Tile24::OW : Tile96::OW; }

// Dynamic tail of the fused path on the 16-lane tile (relmc_eval_kernel phase B, relmc_tail_replay_kernel): the plan of a launch of n
// scenarios on `waves` wavefronts.  Wavefront w owns the groups [begin(w), end(w)) of four scenarios; T = kTailGroups if every wavefront
// owns at least 2 T groups, else 0 (the launch is the static one).  Phase A of w runs [begin(w), end(w) - T); item p of the claim counter,
// 0 <= p < waves * T, is group end(p % waves) - T + p / waves.
#ifndef RELMC_TAIL_GROUPS
#define RELMC_TAIL_GROUPS 8
#endif
constexpr int kTailGroups = RELMC_TAIL_GROUPS;
struct TailPlan {
    int64_t ngroups, waves; int T;
    TailPlan(int64_t n, int64_t waves_) : ngroups((n + Tile24::SPW - 1) / Tile24::SPW), waves(waves_), T(waves_ > 0 && ngroups / waves_ >= 2 * kTailGroups ? kTailGroups : 0) {}
    int64_t begin(int64_t w) const { return ngroups * w / waves; }
    int64_t end(int64_t w) const { return ngroups * (w + 1) / waves; }
    int64_t cut(int64_t w) const { return end(w) - T; }
    int64_t items() const { return waves * T; }
    int64_t owner(int64_t p) const { return p % waves; }
    int64_t group(int64_t p) const { return end(p % waves) - T + p / waves; }
};

// ---- relmc_retry.hip ----------------------------------------------------------------------------------------------------------
constexpr uint32_t kFailCapMin = 4096, kFailCapSteady = 1u << 20, kFailCapMax = 1u << 26;
uint32_t fail_cap_for(int64_t call_units);
int fail_list_ensure(relmc_ctx* ctx, uint32_t cap);
int fail_count_ensure(relmc_ctx* ctx);           // the two count words exist (zeroed when they are created)
// one re-evaluated unit, its meta word (status | relaxed << 2 | iterations << 8) decoded once
struct RetryUnit {
    unsigned long long unit; long long weight; const uint32_t* mask;
    double dns; int32_t meta; int32_t status, iters; bool island_rule;      // island_rule: an island needed Pmin relaxation / decommit (relmc_acc.n_infeasible)
    const double* nodal;
};
struct RetryOut {
    std::vector<FailRec> rec; std::vector<double> dns, nodal; std::vector<int32_t> meta; size_t nb = 0;
    size_t size() const { return rec.size(); }
    RetryUnit operator[](size_t r) const
    {
        const int32_t m = meta[r];
        return {rec[r].unit, (long long)rec[r].weight, rec[r].mask, dns[r], m, m & 3, (int32_t)((uint32_t)m >> 8), (m & 4) != 0, &nodal[r * nb]};
    }
};
int alt_ensure(relmc_ctx* ctx, int v);
int fail_arm(relmc_ctx* ctx, EvalArgs& a, int64_t unit_base, bool reset, int64_t call_units);
// One first-attempt launch of relmc_eval_kernel<mode> and its collection, the protocol of every HL2 entry point (`who`, for the message): the list
// armed for the call_units units of the call (unit_base: the launch's first), the launch, then -- acc != nullptr -- the reduction of its partial
// records, and the accumulators and the listed count back through the context's pinned words in ONE synchronisation.
struct Collected {
    uint32_t listed = 0; bool armed = false;       // units the launch listed (may exceed the list's capacity); armed: there is a list (not sw.no_retry)
    double ms = 0.0;                               // the launch's kernel time (ctx->last_kernel_ms as well)
    const uint32_t* known() const { return armed ? &listed : nullptr; }      // fail_retry's known_count
};
int eval_collect(relmc_ctx* ctx, const char* who, int mode, EvalArgs& a, int64_t unit_base, int64_t call_units, relmc_acc* acc, Collected& c);
using ScaleFn = std::function<double(unsigned long long)>;          // unit -> load scale factor of a re-evaluated unit
// known_count (optional): the number of listed units if the caller has already copied it back with its results; ms (optional)
int fail_retry(relmc_ctx* ctx, const relmc_solver_opts& o, double fail_threshold, const ScaleFn* scale, RetryOut& out, double* ms, const uint32_t* known_count = nullptr);
void acc_add_unit(relmc_acc* acc, const RetryUnit& u, int nb, int ncomp, double fail_threshold);
inline void acc_add_retry(relmc_acc* acc, const RetryOut& ro, int ncomp, double fail_threshold)      // every re-evaluated unit, in list order
{
    for (size_t r = 0; r < ro.size(); ++r) acc_add_unit(acc, ro[r], (int)ro.nb, ncomp, fail_threshold);
}

// ---- relmc_simulate.hip -------------------------------------------------------------------------------------------------------
int pipe_run(relmc_ctx* ctx, const uint8_t* states, const double* load_scale, int64_t n, const relmc_solver_opts& o, double fail_threshold,
             double* dns, double* nodal, int32_t* status, int32_t* iters);
int nsq_accumulate_impl(relmc_ctx* ctx, uint64_t seed, uint64_t first_index, int64_t n, const relmc_solver_opts* opts, relmc_acc* acc_out, double* dns_dev);
// relmc_mc_simulation_dev itself; n_infeasible_out (optional): how many of the n states needed an island rule (relmc_acc.n_infeasible), which no
// per-state output carries -- from the launch's partial records and the re-evaluated units' meta words
int mc_simulation_dev_impl(relmc_ctx* ctx, const uint8_t* states_dev, int64_t n, const relmc_solver_opts* opts, double* dns_dev, double* nodal_dev,
                           int32_t* status_dev, int32_t* iters_dev, int64_t* n_infeasible_out);

// ---- relmc_nsq_run.hip --------------------------------------------------------------------------------------------------------
constexpr int64_t kStretch = 1 << 18, kStretchMaxBatch = 32768;      // samples a stretch holds at most; batches above the second are not stretched
inline int64_t stretch_per(int64_t batch) { return kStretch / batch * batch; }      // the longest stretch in whole batches
// Length of the stretch that follows `done` samples at `beta` (no context, no HIP); final: sized to end the run.  per: the longest allowed;
// round: samples of one round of the fused grid, below whose multiples other stretches end (0 = do not snap: the database form)
struct Stretch { int64_t len; bool final; };
Stretch stretch_length(int64_t batch, int64_t done, double beta, double beta_limit, int64_t per, int64_t round);

// ---- relmc_database.hip -------------------------------------------------------------------------------------------------------
int db_accumulate(relmc_ctx* ctx, relmc_acc* acc_out);
int db_rewind(relmc_ctx* ctx, int64_t rows0, int64_t samples0);      // back to the first rows0 rows with the counts saved in ctx->db.snap
int db_snapshot(relmc_ctx* ctx);                                    // saves the counts of the present rows into ctx->db.snap
int db_sample_dns(relmc_ctx* ctx, uint64_t seed, uint64_t first_index, int64_t m, double* dns_dev);   // dns of every sample of a range from its row

// ---- relmc_comm.hip -----------------------------------------------------------------------------------------------------------
void comm_free(relmc_ctx* ctx);                   // stops the watchdog, destroys the RCCL communicator
inline int comm_ranks(const relmc_ctx* ctx) { return (ctx->comm || ctx->host_allreduce) ? ctx->comm_nranks : 1; }
// sum over the ranks of a vector of doubles, in place (the all-gather of the sequential loop: every rank fills its own slots, zeros elsewhere --
// x + 0 + ... + 0 is exact).  RCCL: one ncclAllReduce; host collective: through the registered relmc_acc all-reduce, 130 doubles per call
int comm_allreduce_f64(relmc_ctx* ctx, double* buf, int64_t count);

// ---- relmc_screen.hip ---------------------------------------------------------------------------------------------------------
int screen_build(relmc_ctx* ctx, const relmc_case_desc* d);          // relmc_case_load: PTDF / LODF tables of the certificate
// samples [first_index, first_index + m): masks of the uncovered ones in ctx->screen.keys (own position), their ascending positions in ctx->screen.idx
int screen_prepass_nsq(relmc_ctx* ctx, uint64_t seed, uint64_t first_index, int64_t m, uint32_t* n_surv, double* ms);
int screen_gather_keys(relmc_ctx* ctx, uint32_t n_surv, uint32_t* keys_out);               // the uncovered samples' masks of the last screen_prepass_nsq, packed in sample order
int screen_prepass_rows(relmc_ctx* ctx, int64_t first, int64_t n, uint32_t* n_surv);      // new database rows: certified ones filled in, the others listed
int screen_seq_compact(relmc_ctx* ctx, const uint32_t* masks, int n_years, uint16_t* hours, uint32_t* counts, uint32_t* ncont);
constexpr int64_t kScreenChunk = (int64_t)1 << 22;                   // samples per pre-pass of the fused path (its buffers: 4 OW + 5 bytes per sample)

// ---- relmc_seq.hip ------------------------------------------------------------------------------------------------------------
// relmc_seq_events' accumulator and histogram (optional) zeroed: what seq_events_device expects to be handed
inline void seq_events_zero(relmc_seq_event_acc* ev_acc, int32_t n_dur_bins, int64_t* dur_hist_host)
{
    std::memset(ev_acc, 0, sizeof(*ev_acc));
    if (dur_hist_host) std::memset(dur_hist_host, 0, sizeof(int64_t) * n_dur_bins);
}
// Loss events of device hours curt[n_years][hpy] with masks[n_years][hpy][mw] (relmc_seq_events behind its relmc_seq_years step;
// relmc_debug_seq_events on uploaded hours): count -> offsets -> fill -> reduce, outputs as relmc_seq_events documents them (ev_acc->years
// = n_years).  total_hint: the number of events if the caller knows it (the years' nlc), which saves the synchronisation that reads it
// back; -1 = read it.  Adds the kernels' time to *ms.  The caller hands in zeroed outputs (seq_events_zero).
int seq_events_device(relmc_ctx* ctx, const char* who, const double* curt, const uint32_t* masks, int n_years, int hpy, int mw, double threshold,
                      int64_t total_hint, relmc_seq_event_acc* ev_acc, int32_t n_dur_bins, int64_t* dur_hist_host, int64_t events_cap,
                      relmc_seq_event* events_host, double* ms);

}  // namespace relmc_host
