/*
 * relmc.h — C ABI of the MI355X-native non-sequential Monte Carlo HL2 engine.
 *
 * Drop-in boundary for the hot path of Matrixeigs/PowerSystemsReliabilityAssessment
 * (SURVEY.md §8b).  The reference has no FFI of its own: its "operator API" is three
 * MATLAB signatures, which the entry points below replace one for one:
 *
 *   relmc_case_load        <- loadcase + load model + failprob
 *                             (Montecarlo_nsq_single/nsqMain.m:42,121-153,167; failprob.m:1-41)
 *   relmc_mc_sampling      <- eqstatus = mc_sampling(U, n, Ng, Nl)          (mc_sampling.m:2)
 *   relmc_mc_simulation    <- [dns, nodal_dns] = mc_simulation(state, ...)  (mc_simulation.m:1),
 *                             batched over states (the parfor of nsqMain.m:257-263)
 *   relmc_nsq_accumulate   <- one pass of the main loop body, fused sample -> evaluate -> reduce
 *                             (nsqMain.m:212, 257-263, 269-278 folded into per-sample sums)
 *   relmc_nsq_indices      <- the estimators of nsqMain.m:282-301, 348-349, 366-376
 *   relmc_nsq_run          <- the whole `while beta > beta_limit` loop, nsqMain.m:208-318
 *
 * Conventions: plain C, no C++ or torch types; every buffer is owned by the caller and is
 * not retained after the call returns; row-major arrays; all floating point is fp64;
 * return value 0 = ok, <0 = relmc_status error (text via relmc_last_error); calls on one
 * context are blocking and not re-entrant, distinct contexts are independent.  One context
 * drives ONE GPU (one process per GPU; multi-GPU runs shard the global scenario index range
 * and all-reduce relmc_acc).  There is NO CPU fallback: if no HIP device
 * is usable every entry point fails with RELMC_ERR_NO_DEVICE.
 */
#ifndef RELMC_H
#define RELMC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RELMC_MAX_BUS 128
#define RELMC_MAX_COMP 256

typedef enum {
    RELMC_OK = 0,
    RELMC_ERR_INVALID = -1,      /* bad argument */
    RELMC_ERR_NO_DEVICE = -2,    /* no usable HIP device / HIP runtime error at create */
    RELMC_ERR_HIP = -3,          /* HIP runtime error (see relmc_last_error) */
    RELMC_ERR_UNSUPPORTED = -4,  /* case larger than the compiled kernel tiles */
    RELMC_ERR_NO_CASE = -5       /* relmc_case_load has not been called */
} relmc_status;

/* How states that leave a bus with no in-service branch are evaluated.
 * Known deviation: a MULTI-bus island without the reference bus also makes MATPOWER's KKT matrix singular (a constant angle
 * shift of the island is a null vector), but what MATLAB's `\` returns on that nearly singular matrix cannot be known
 * here; such states (about 1e-6 per RTS-24 sample) are solved island-aware under BOTH policies and are not claimed to
 * emulate the reference.  relmc_acc.n_infeasible / n_singular let a caller bound how many states any policy touched. */
typedef enum {
    RELMC_REFERENCE_EMULATE = 0, /* MATPOWER/MIPS fails in iteration 1, the start point is
                                    consumed unchecked (mc_simulation.m:41,54): dns = load/2 */
    RELMC_PHYSICAL = 1           /* island-aware LP: every island gets its own angle reference */
} relmc_singular_policy;

/* Per-scenario solver status. */
typedef enum {
    RELMC_ST_CONVERGED = 0,
    RELMC_ST_MAXIT = 1,          /* max_it reached (MIPS eflag 0)       */
    RELMC_ST_NUMFAIL = 2,        /* MIPS "numerically failed" (eflag -1) */
    RELMC_ST_SINGULAR = 3        /* isolated bus under RELMC_REFERENCE_EMULATE */
} relmc_scenario_status;

typedef struct relmc_ctx relmc_ctx;

/* Study case = MATPOWER case after the load model of nsqMain.m:121-153, 0-based indices.
 * Injections are the LP's generator columns in MATPOWER order: ng real generators then nd
 * virtual generators (one per load bus: Pmax = 0, Pmin = -Pd, cost 1). */
typedef struct {
    double base_mva;
    int32_t nb, ng, nl, nd;
    int32_t ref_bus;
    const double* bus_pd;     /* [nb]    MW, original bus loads                    */
    const int32_t* inj_bus;   /* [ng+nd]                                           */
    const double* inj_pmin;   /* [ng+nd] MW                                        */
    const double* inj_pmax;   /* [ng+nd] MW                                        */
    const double* inj_cost;   /* [ng+nd] linear cost c1 ($/MWh)                    */
    const int32_t* br_from;   /* [nl]                                              */
    const int32_t* br_to;     /* [nl]                                              */
    const double* br_b;       /* [nl]    1/(x*tap) p.u. (makeBdc)                  */
    const double* br_rate;    /* [nl]    MW, 0 = unconstrained                     */
    const double* unavail;    /* [ng+nl] failure probabilities (failprob.m:39)     */
    const uint8_t* always_up; /* [ng+nl] 1 = forced available (mc_sampling.m:40-41) */
    double total_load;        /* TestSystem.load, nsqMain.m:125                    */
} relmc_case_desc;

/* MIPS options as MATPOWER sets them for OPF_ALG_DC=200 (nsqMain.m:185-186). */
typedef struct {
    int32_t singular_policy;  /* relmc_singular_policy */
    int32_t max_it;           /* 150 */
    double feastol;           /* 5e-6 (opf.violation) */
    double gradtol;           /* 1e-6 */
    double comptol;           /* 1e-6 */
    double costtol;           /* 1e-6 */
    double xi;                /* 0.99995 */
    double sigma;             /* 0.1 */
    double z0;                /* 1 */
    double alpha_min;         /* 1e-8 */
    double max_stepsize;      /* 1e10 */
    int32_t screen;           /* 0 (default): every unit goes through the interior point.  1: zero-curtailment pre-screen: a unit
                                 for which an explicit dispatch serves all load -- units in service loaded proportionally between Pmin and Pmax, DC
                                 flows through the base-topology PTDF (one or two lines out: + the outage system's corrections) inside or on every rating -- has LP optimum 0, so the
                                 reference's outputs for it are exactly (0, zeros) (mc_simulation.m:57-59, 65) and it is counted without being solved.
                                 Every output but the iteration statistics is the one of screen = 0 (of its converged solves: a unit the interior point
                                 would have left non-converged is counted with the proven optimum); relmc_acc.n_screened counts the skipped units.
                                 Honoured by the fused pass (relmc_nsq_accumulate, relmc_nsq_run), by the per-batch dedupe
                                 (relmc_nsq_accumulate_distinct: only the uncovered samples are sorted, their distinct states solved), by the new
                                 rows of the state database (relmc_nsq_db_batch: a certified row carries 0 iterations) and by the sequential
                                 track's contingency hours at their own load factor (relmc_seq_years, relmc_seq_run); relmc_mc_simulation
                                 solves every state it is handed. */
    int32_t reserved;         /* 0 */
} relmc_solver_opts;

/* Additive accumulators of one scenario range (what is all-reduced across GPUs). */
typedef struct {
    int64_t n;                /* scenarios evaluated                                  */
    int64_t n_fail;           /* dns > 1e-4 (nsqMain.m:270)                            */
    int64_t n_singular;       /* RELMC_ST_SINGULAR                                     */
    int64_t n_infeasible;     /* states where an island needed Pmin relaxation / decommit */
    int64_t n_nonconverged;   /* RELMC_ST_MAXIT or RELMC_ST_NUMFAIL                    */
    int64_t sum_iters;        /* IPM iterations                                        */
    int64_t comp_fail[RELMC_MAX_COMP]; /* sum over failed scenarios of state_k (nsqMain.m:373-376) */
    int64_t n_screened;       /* of n: certified zero-curtailment by the pre-screen and not solved (relmc_solver_opts.screen) */
    double sum_dns;           /* sum dns      (nsqMain.m:286)                          */
    double sum_dns2;          /* sum dns^2    (for beta, nsqMain.m:299-301)            */
    double sum_nodal[RELMC_MAX_BUS];   /* sum nodal_dns (nsqMain.m:348)               */
} relmc_acc;

/* Reliability indices (nsqMain.m:282-301, 348-349, 366-376). */
typedef struct {
    int64_t n;
    double edns;              /* MW                       */
    double lole;              /* h/yr = plc*hours_per_year */
    double plc;
    double beta;              /* CoV of EDNS              */
    double eens;              /* MWh/yr = edns*hours_per_year */
    double mean_iters;
    double nodal_eens[RELMC_MAX_BUS];        /* MW (the reference's nodal_eens; x8760 in its CSV) */
    double comp_importance[RELMC_MAX_COMP];  /* P(component down | system failure) */
} relmc_indices;

typedef struct {
    double beta_limit;        /* nsqMain.m:60  (0.0017) */
    int64_t max_samples;      /* nsqMain.m:61  (1e5)    */
    int64_t batch;            /* scenarios per convergence check (nsqMain.m:62 uses 100) */
    uint64_t seed;
    double hours_per_year;    /* 8760, nsqMain.m:292 */
    relmc_solver_opts solver;
    /* optional history buffers (may be NULL); capacity in checkpoints */
    int64_t history_cap;
    double* beta_history;
    double* edns_history;
    double* lole_history;
    double* plc_history;
    int32_t distinct_states;  /* 0 (default): solve every sample.
                                 1: evaluate every distinct state of a batch once and count multiplicities (the
                                    reference's dedupe, nsqMain.m:220-229, per batch).
                                 2: the reference's persistent unique-state database (nsqMain.m:91-99, 220-278): states
                                    seen in an earlier batch only bump their count, only new states are solved, and the
                                    indices are recomputed from all rows after every batch (:282-301).  The run starts
                                    from an empty database (relmc_db_reset).
                                 The estimators are identical in all three. */
} relmc_nsq_opts;

typedef struct {
    relmc_acc acc;
    relmc_indices idx;
    int64_t checkpoints;      /* history entries written = min(batches, history_cap) */
    int32_t converged;        /* beta <= beta_limit */
    double wall_seconds;      /* host wall time of the loop */
    double kernel_seconds;    /* HIP-event time of the fused kernels */
    int64_t batches;          /* convergence checks made (passes of the nsqMain.m:208 loop) */
} relmc_nsq_result;

/* ---- lifetime ---------------------------------------------------------------------- */
int32_t relmc_ctx_create(int32_t device_id, relmc_ctx** out);
void relmc_ctx_destroy(relmc_ctx* ctx);
const char* relmc_last_error(const relmc_ctx* ctx);
const char* relmc_version(void);

/* ---- setup ------------------------------------------------------------------------- */
void relmc_solver_opts_default(relmc_solver_opts* opts);
void relmc_nsq_opts_default(relmc_nsq_opts* opts);
int32_t relmc_case_load(relmc_ctx* ctx, const relmc_case_desc* desc);
/* integer Bernoulli thresholds floor(U*2^32) the sampler compares against; out[ng+nl] */
int32_t relmc_case_thresholds(const relmc_ctx* ctx, uint32_t* out);

/* ---- mc_sampling (mc_sampling.m:2) -------------------------------------------------- */
/* eqstatus[n x (ng+nl)] row-major, 1 = failed.  Deterministic in (seed, global index). */
int32_t relmc_mc_sampling(relmc_ctx* ctx, uint64_t seed, uint64_t first_index, int64_t n,
                          uint8_t* eqstatus_host);
int32_t relmc_mc_sampling_dev(relmc_ctx* ctx, uint64_t seed, uint64_t first_index, int64_t n,
                              uint8_t* eqstatus_dev);

/* ---- mc_simulation (mc_simulation.m:1), batched ------------------------------------- */
/* states[n x (ng+nl)]; dns[n]; nodal[n x nb]; status[n] / iters[n] may be NULL. */
int32_t relmc_mc_simulation(relmc_ctx* ctx, const uint8_t* states_host, int64_t n,
                            const relmc_solver_opts* opts, double* dns_host, double* nodal_host,
                            int32_t* status_host, int32_t* iters_host);
/* same with every buffer already resident in this device's HBM */
int32_t relmc_mc_simulation_dev(relmc_ctx* ctx, const uint8_t* states_dev, int64_t n,
                                const relmc_solver_opts* opts, double* dns_dev, double* nodal_dev,
                                int32_t* status_dev, int32_t* iters_dev);

/* ---- fused sample -> evaluate -> reduce (nsqMain.m:208-318 loop body) ---------------- */
/* Evaluates global scenarios [first_index, first_index+n) and returns their accumulators. */
int32_t relmc_nsq_accumulate(relmc_ctx* ctx, uint64_t seed, uint64_t first_index, int64_t n,
                             const relmc_solver_opts* opts, relmc_acc* acc_out);
/* HIP-event duration (ms) of the most recent fused / simulation kernel on the ctx stream */
/* The same accumulators through the reference's dedupe (nsqMain.m:220-245): sample the range, sort the outage masks on
 * the device, evaluate each distinct state once weighted by its multiplicity.  *n_distinct_out (optional) = states solved.
 * With opts->screen = 1 the pre-screen's certificate runs first and only the uncovered samples are sorted and solved.
 * relmc_last_kernel_ms then covers sampling + sort + evaluation. */
int32_t relmc_nsq_accumulate_distinct(relmc_ctx* ctx, uint64_t seed, uint64_t first_index, int64_t n,
                                      const relmc_solver_opts* opts, relmc_acc* acc_out, int64_t* n_distinct_out);
int32_t relmc_last_kernel_ms(const relmc_ctx* ctx, double* ms);

/* ---- persistent unique-state database (nsqMain.m:91-99, 220-278) ------------------------- */
/* The reference keeps every distinct state it has ever sampled in `state_database` (columns: Ng+Nl component states |
 * count | dns | failure flag | Nb nodal values, nsqMain.m:91-99).  Per batch it removes duplicates (:220-229), bumps the
 * counts of states already in the database (:232-245), evaluates only the new ones (:257-263), appends them (:269-278)
 * and recomputes the indices from all rows (:282-301).  The same on the device: rows in HBM, an open-addressing table of
 * row ids (probed per sample once the database is warm; only the misses are sorted and deduplicated), new rows appended in
 * the order of first appearance in the sample stream (unique(...,'stable')), so the database and every sum over it depend
 * on (seed, samples drawn) only, not on the batch size.
 *   relmc_db_reset       empty database (relmc_case_load does the same)
 *   relmc_nsq_db_batch   one pass of the loop body over samples [first_index, first_index + n); acc_out (optional) =
 *                        accumulators of the WHOLE database afterwards (cumulative, not the batch's increment)
 *   relmc_db_accumulate  the accumulators of the whole database again (no sampling)
 *   relmc_db_size        rows and samples held
 *   relmc_db_export      rows [first_row, first_row + n_rows) in the reference's column layout (RELMC_ERR_INVALID, database untouched, unless
 *                        0 <= first_row, 0 <= n_rows and first_row + n_rows <= rows; an empty range is fine); any output may be NULL:
 *                        states[n x (ng+nl)], count[n], dns[n], flag[n] (dns > 1e-4, :270), nodal[n x nb], status[n], iters[n],
 *                        relaxed[n] (bit 0 = an island rule relaxed Pmin or decommitted units: the row counts in n_infeasible; bit 1 = the row was
 *                        certified by the pre-screen and never solved: it counts in n_screened)
 *   relmc_db_import      resume: exported rows back into an EMPTY database, same order (the table of row ids is rebuilt); the next
 *                        relmc_nsq_db_batch / relmc_nsq_run(distinct_states = 2) continues as if the run had never stopped.
 *                        opts = the solver options the rows were computed under (NULL = defaults); status / iters / relaxed may be NULL.
 *                        Every row is checked on the host before anything is copied: one row per state (a state on two rows would split its
 *                        count and break the independence of the batch size), iters in [0, 2^23) (the row's meta word keeps it above bit 8),
 *                        counts >= 1.  A violation returns RELMC_ERR_INVALID with relmc_last_error naming the first offending row and leaves
 *                        the database empty and usable.
 * After an error return of relmc_nsq_db_batch on a non-empty database the counts of known rows may have advanced without their
 * samples: the database then refuses every call but relmc_db_reset (and relmc_case_load) with RELMC_ERR_INVALID. */
typedef struct {
    int64_t rows;             /* distinct states in the database (database_row_count)     */
    int64_t samples;          /* samples they stand for (sum of the count column)          */
    int64_t new_rows;         /* states evaluated by this call (num_new_states, :255)       */
    int64_t batch_distinct;   /* distinct states among this call's samples that went through the dedupe: all of
                                 them on an empty database, only the misses of the per-sample probe on a warm one */
} relmc_db_stats;
int32_t relmc_db_reset(relmc_ctx* ctx);
int32_t relmc_nsq_db_batch(relmc_ctx* ctx, uint64_t seed, uint64_t first_index, int64_t n,
                           const relmc_solver_opts* opts, relmc_acc* acc_out, relmc_db_stats* stats_out);
int32_t relmc_db_accumulate(relmc_ctx* ctx, relmc_acc* acc_out);
int32_t relmc_db_size(const relmc_ctx* ctx, int64_t* rows_out, int64_t* samples_out);
int32_t relmc_db_export(relmc_ctx* ctx, int64_t first_row, int64_t n_rows, uint8_t* states_host, int64_t* count_host,
                        double* dns_host, int32_t* flag_host, double* nodal_host, int32_t* status_host, int32_t* iters_host,
                        uint8_t* relaxed_host);
int32_t relmc_db_import(relmc_ctx* ctx, const relmc_solver_opts* opts, int64_t n_rows, const uint8_t* states_host,
                        const int64_t* count_host, const double* dns_host, const double* nodal_host, const int32_t* status_host,
                        const int32_t* iters_host, const uint8_t* relaxed_host);

/* ---- multi-GPU: the path's single collective (the reference's parfor, nsqMain.m:257-263) ------------ */
/* One process per GPU, one context per process.  Scenarios shard by global index (any contiguous split of
 * [first_index, first_index + n) over the ranks); at a convergence check every rank calls relmc_comm_allreduce_acc on the
 * accumulators of its slice: ONE grouped RCCL all-reduce(sum) over xGMI (int64 counters and fp64 sums in their own types).
 * The communicator is bootstrapped like any RCCL communicator: rank 0 calls relmc_comm_unique_id and hands the 128 bytes
 * to the other ranks by the host's own means (file, socket, MPI, Julia Distributed, torch store), then every rank calls
 * relmc_comm_init.  RCCL is bound at run time (dlopen): hosts that never call these need no RCCL installed. */
#define RELMC_COMM_ID_BYTES 128
int32_t relmc_comm_unique_id(uint8_t id_out[RELMC_COMM_ID_BYTES]);
int32_t relmc_comm_init(relmc_ctx* ctx, int32_t nranks, int32_t rank, const uint8_t id[RELMC_COMM_ID_BYTES]);
int32_t relmc_comm_allreduce_acc(relmc_ctx* ctx, relmc_acc* acc_inout);
int32_t relmc_comm_destroy(relmc_ctx* ctx);
/* A host that brings its own transport (MPI, Julia Distributed, torch.distributed over gloo) registers it instead of an RCCL
 * communicator: fn(user, acc) leaves the sum over all ranks in *acc on every rank (0 = ok) and is called in the same order on every
 * rank.  With either kind of communicator of more than one rank in the context, relmc_nsq_run IS the multi-rank loop: every batch of
 * the global sample stream is split contiguously over the ranks, one all-reduce per batch, every rank returns the same result
 * (nsqMain.m:208-318 around the parfor of :257-263); relmc_comm_allreduce_acc goes through the registered collective as well.
 * relmc_comm_info: kind 0 = none, 1 = RCCL (ranks / rank as ncclCommCount / ncclCommUserRank report them), 2 = host collective;
 * all-reduces issued through this context (of relmc_acc, and of vectors: relmc_comm_allreduce_f64 counts once per call) and the wall time
 * spent in them.  Any output may be NULL. */
typedef int32_t (*relmc_allreduce_fn)(void* user, relmc_acc* acc_inout);
int32_t relmc_comm_set_host_allreduce(relmc_ctx* ctx, int32_t nranks, int32_t rank, relmc_allreduce_fn fn, void* user);
/* Optional vector transport of a host collective (after relmc_comm_set_host_allreduce): fn(user, buf, count) leaves the sum over all ranks of
 * `count` doubles in buf on every rank (0 = ok).  relmc_comm_allreduce_f64 -- the all-gather of the sequential loop's annual indices
 * (seqMain.m:112-133) and the per-checkpoint sums of relmc_nsq_run's stretches -- is then ONE callback per call instead of count / 130 through the
 * relmc_acc callback.  NULL removes it. */
typedef int32_t (*relmc_allreduce_f64_fn)(void* user, double* buf_inout, int64_t count);
int32_t relmc_comm_set_host_allreduce_f64(relmc_ctx* ctx, relmc_allreduce_f64_fn fn, void* user);
int32_t relmc_comm_info(const relmc_ctx* ctx, int32_t* kind_out, int32_t* nranks_out, int32_t* rank_out, int64_t* calls_out,
                        double* seconds_out);
/* Wall-clock guard.  relmc_comm_init and every collective issued through the context (RCCL or the host's callback) must finish within
 * `seconds` (default 120; <= 0 switches the guard off): a peer that never arrives cannot be waited out from inside a collective, so on
 * expiry the rank prints its rank / rank count / pid / device / PCI bus id and what it was waiting for on stderr and ends the process with
 * exit code 86 -- a multi-GPU job that would hang for the launcher's own timeout becomes a diagnosis within two minutes. */
int32_t relmc_comm_set_timeout(relmc_ctx* ctx, double seconds);
/* Sum over the ranks of `count` doubles, in place (same result on every rank).  The sequential loop all-gathers its annual indices with it
 * (every rank fills its own slots of a zeroed vector: x + 0 + ... + 0 is exact).  RCCL: one ncclAllReduce; a host collective: one call of
 * the vector transport (relmc_comm_set_host_allreduce_f64) if there is one, else the registered relmc_acc all-reduce, 130 doubles per call. */
int32_t relmc_comm_allreduce_f64(relmc_ctx* ctx, double* buf_inout, int64_t count);
/* PCI bus id of the GPU the context drives ("0000:c1:00.0", cap >= 16): what a multi-rank host gathers to show its ranks sit on DISTINCT devices */
int32_t relmc_device_pci_bus_id(const relmc_ctx* ctx, char* out, int32_t cap);

/* ---- estimators (host arithmetic, no device) ---------------------------------------- */
void relmc_acc_zero(relmc_acc* acc);
void relmc_acc_merge(relmc_acc* dst, const relmc_acc* src);
void relmc_nsq_indices(const relmc_acc* acc, int32_t nb, int32_t ncomp, double hours_per_year,
                       relmc_indices* out);

/* ---- HL1 copper-sheet non-sequential MC --------------------------- */
/* Mirrors GeneratingAdequacy/PowerSystemAdequacy.jl:169-208 run_non_sequential_mc(gens, load,
 * iterations): per iteration one fleet state (unit g is down iff draw < FOR_g, i.e. up iff
 * rand() >= for_rate, :183-185), available capacity, then the whole hourly load curve is swept:
 * hours with cap < load and their deficit (:191-197).  Unit g is down iff draw < thr_g, thr_g = floor(for_rate_g * 2^32) clamped to
 * [0, 2^32 - 1] (so for_rate 1 leaves a unit up with probability 2^-32).  The deficit of an iteration is the exact sum of
 * (load - cap) over its loss hours up to a few ulp of the result: the load curve's suffix sums are held in double-double.
 * Input rule of the four HL1 load calls (relmc_hl1_load, relmc_hl1_seq_load, relmc_hl1_area_load, relmc_hl1_plan_load): every capacity
 * is finite, every for_rate (relmc_hl1_load, relmc_hl1_plan_load) lies in [0, 1], every hourly load is finite; a call that breaks the
 * rule changes nothing and returns RELMC_ERR_INVALID with relmc_last_error naming the unit or the hour (and the area). */
typedef struct {
    int64_t n;                /* iterations                                 */
    double sum_lole;          /* sum over iterations of loss hours          */
    double sum_eue;           /* sum over iterations of unserved energy MWh */
    double sum_lole2, sum_eue2;
} relmc_hl1_acc;
int32_t relmc_hl1_load(relmc_ctx* ctx, int32_t ngen, const double* capacity_mw, const double* for_rate,
                       int32_t nhours, const double* hourly_load_mw);
/* iter_lole / iter_eue: optional host buffers [n] with the per-iteration values (history, :202-204) */
int32_t relmc_hl1_nsq(relmc_ctx* ctx, uint64_t seed, uint64_t first_index, int64_t n, relmc_hl1_acc* acc,
                      double* iter_lole_host, double* iter_eue_host);

/* ---- HL1 copper-sheet sequential MC (PowerSystemAdequacy.jl:214-268 run_sequential_mc) ------------------- */
/* Two-state exponential units sampled at integer steps.  A chain of Y years has steps n = 1 .. Y*H (step n is hour (n-1) mod H of
 * chain year (n-1) div H); the fleet state carries over from year to year.  With T_1 < T_2 < ... a unit's cumulative transition
 * times, its state at step n is its start state toggled once for every T_j <= n.
 * Draw e of unit k in chain c: U = (philox4x32_10(ctr = (c_lo, c_hi, k | 0x40000000, e >> 2), key = (seed_lo, seed_hi))[e & 3] + 0.5) / 2^32.
 * Durations -mttf*ln U (UP) / -mttr*ln U (DOWN) in fp64, T_{j+1} = T_j + duration, product and sum each rounded (no FMA).
 *   RELMC_HL1_START_ALL_UP:     every unit UP at time 0, draw 0 is the first time to failure (the reference, :223-224)
 *   RELMC_HL1_START_STATIONARY: draw 0 decides the start state (DOWN iff U < mttr / (mttf + mttr)), durations from draw 1 on
 * Per step: cap_avail = sum of the UP units' capacities in ascending unit order; loss iff cap_avail < load (strict), deficit
 * load - cap_avail (:249-256).  Per year: loss hours, EUE, and loss events = steps where the loss flag rises (step 1 of the chain
 * counts if it is a loss hour; an event that runs across a year boundary counts once, in the year it started). */
#define RELMC_HL1_START_ALL_UP     0
#define RELMC_HL1_START_STATIONARY 1
typedef struct { double lole, eue, lolf; } relmc_hl1_seq_year;            /* loss hours, MWh, loss events of one simulated year */
typedef struct {
    int64_t years;                                                          /* simulated years summed */
    double sum_lole, sum_eue, sum_lolf, sum_lole2, sum_eue2, sum_lolf2;
} relmc_hl1_seq_acc;
/* Fleet (ngen <= 128 units, mttf / mttr in hours, finite and > 0) and the hourly load curve of one year (nhours >= 1).  Held apart
 * from relmc_hl1_load's model: neither call disturbs the other. */
int32_t relmc_hl1_seq_load(relmc_ctx* ctx, int32_t ngen, const double* capacity_mw, const double* mttf_h, const double* mttr_h,
                           int32_t nhours, const double* hourly_load_mw);
/* chains [first_chain, first_chain + n_chains), each years_per_chain consecutive years; years_host: optional [n_chains * years_per_chain],
 * chain-major.  Results depend on (seed, chain, start, years_per_chain, data) only, not on how a chain range is split into calls; the
 * sums of `acc` are taken in a fixed order, so a repeated call is bitwise identical. */
int32_t relmc_hl1_seq(relmc_ctx* ctx, uint64_t seed, uint64_t first_chain, int64_t n_chains, int32_t years_per_chain,
                      int32_t start, relmc_hl1_seq_acc* acc, relmc_hl1_seq_year* years_host);

/* ---- loss events of the HL1 sequential chronology: how often failures occur and how long they last (seqMain.m:15-16) ---- */
/* The chronology is relmc_hl1_seq's, word for word (model of relmc_hl1_seq_load, draws, start rules, no FMA, DOWN on steps
 * [ceil(T_odd), ceil(T_even)), cap_avail over the UP units in ascending order, loss iff cap_avail < load[(n-1) mod H], deficit
 * load - cap_avail): under one seed, chain c sees exactly the fleet history of chain c of relmc_hl1_seq.
 * A loss event of a chain is a maximal run of consecutive loss steps among its steps 1 .. Y*H.  start_step n0 is 1-based along the chain,
 * duration D the number of steps, energy E the sum of the steps' deficits, peak P the largest of them.  A run continues across a year
 * boundary (it belongs to the year it starts in, as relmc_hl1_seq's lolf); a run that reaches step Y*H ends there and is counted as
 * censored (it is an event like any other in every other field).  So `events` equals relmc_hl1_seq's sum_lolf and sum_dur its sum_lole
 * exactly, and sum_energy its sum_eue up to the order of summation. */
typedef struct {
    int64_t chain;            /* index relative to first_chain */
    int64_t start_step;       /* 1-based along the chain */
    int64_t duration;         /* steps */
    double energy_mwh, peak_mw;
} relmc_hl1_event;
typedef struct {
    int64_t years, events, censored, sum_dur, sum_dur2, max_dur;            /* years = simulated years; sums and maxima over the events */
    double sum_energy, sum_energy2, max_energy, max_peak;
} relmc_hl1_event_acc;
/* chains [first_chain, first_chain + n_chains), each years_per_chain consecutive years, of the model loaded by relmc_hl1_seq_load
 * (RELMC_ERR_NO_CASE before that call); arguments are checked as relmc_hl1_seq checks them, n_chains == 0 zeroes the outputs.
 *   dur_hist_host  optional [n_dur_bins], 1 <= n_dur_bins <= 4096 when given (else RELMC_ERR_INVALID): dur_hist_host[d - 1] = events with
 *                  D = d for d < n_dur_bins, the last bin counts D >= n_dur_bins; overwritten with this call's counts
 *   events_host    optional [events_cap], events_cap >= 0 (else RELMC_ERR_INVALID): the first min(acc->events, events_cap) events in
 *                  (chain, start_step) order; acc->events is always the true count, so a caller sees that its buffer was short
 * Every output depends on (seed, chain, start, years_per_chain, data) only: splitting a chain range into calls gives lists that concatenate
 * (with `chain` rebased), integer fields and histograms that add exactly and maxima that combine by max; the floating-point sums are
 * taken in a fixed order, so a repeated call is bitwise identical.  Long chain ranges go in launches of at most ~4M chain years, as in
 * relmc_hl1_seq; relmc_last_kernel_ms covers every launch of the call (the list costs a second walk of the chains). */
int32_t relmc_hl1_seq_events(relmc_ctx* ctx, uint64_t seed, uint64_t first_chain, int64_t n_chains, int32_t years_per_chain,
                             int32_t start, relmc_hl1_event_acc* acc, int32_t n_dur_bins, int64_t* dur_hist_host,
                             int64_t events_cap, relmc_hl1_event* events_host);

/* ---- load sweep on the HL1 sequential chronology: one fleet history against up to 16 load levels (an extension beyond the reference) ---- */
/* The reference evaluates one fleet against one load curve.  A planner also asks how much load a fleet carries at a risk target (PLCC)
 * and what a unit is worth in load (ELCC); both are root searches on risk as a function of load, and this call gives up to 16 points of
 * that function from ONE walk of every chain.
 * The chronology is relmc_hl1_seq's, word for word (model of relmc_hl1_seq_load, draws (seed, chain, k | 0x40000000, event), start rules,
 * no FMA, DOWN on steps [ceil(T_odd), ceil(T_even))): under one seed, chain c of every level sees exactly the fleet history of chain c of
 * relmc_hl1_seq.
 *   load of level j at hour h   L_j(h) = scale_j * load[h] + shift_j, the product and the sum each rounded (numpy's scale * load + shift)
 *   fleet of level j            0: every unit; 1: every unit except those whose bit is set in `withheld` (bit k & 31 of word k >> 5).
 *                               cap_avail of fleet 1 is the same ascending loop over the UP units in which a withheld unit adds 0.0
 *                               (exact), i.e. bitwise the fleet whose withheld capacities were loaded as 0.0
 *   loss iff cap_fleet < L_j(h) (strict), deficit L_j(h) - cap_fleet; per level and year: loss hours, EUE, loss events by relmc_hl1_seq's
 *   rules (step 1 counts, an event across a year boundary counts once, in the year it starts; every level has its own previous-step flag)
 * A level's EUE of a year is summed in relmc_hl1_seq's order, so level (1.0, 0.0, fleet 0) reproduces relmc_hl1_seq's year records bit
 * for bit, and any level those of relmc_hl1_seq on the model loaded with its curve and with the withheld capacities as 0.0.
 * A level's year records depend on (seed, chain, start, years_per_chain, data, that level, withheld) only: not on the other levels, their
 * order, or how a chain range is split into calls.  acc[j] is summed in a fixed order, so a repeated call is bitwise identical. */
#define RELMC_HL1_SWEEP_MAX_LEVELS 16
typedef struct { double scale, shift; int32_t fleet; int32_t reserved; } relmc_hl1_sweep_level;   /* 24 bytes, reserved = 0 */
/* chains [first_chain, first_chain + n_chains), each years_per_chain consecutive years, of the model loaded by relmc_hl1_seq_load
 * (RELMC_ERR_NO_CASE before that call).  RELMC_ERR_INVALID, with relmc_last_error naming the level or the bit, for: a null ctx, levels or
 * acc; n_levels outside 1 .. RELMC_HL1_SWEEP_MAX_LEVELS; a non-finite scale or shift; fleet not 0 or 1; reserved != 0; fleet 1 with
 * withheld == NULL; a withheld bit at or above ngen; anything relmc_hl1_seq refuses.  A refused call changes nothing; n_chains == 0
 * zeroes the outputs.
 *   withheld    optional [4] mask words (128 units)
 *   acc         [n_levels]
 *   years_host  optional [n_levels][n_chains * years_per_chain], level-major, then chain-major
 * Long chain ranges go in launches of at most ~4M year records counted over all levels; relmc_last_kernel_ms covers every launch. */
int32_t relmc_hl1_seq_sweep(relmc_ctx* ctx, uint64_t seed, uint64_t first_chain, int64_t n_chains, int32_t years_per_chain,
                            int32_t start, int32_t n_levels, const relmc_hl1_sweep_level* levels,
                            const uint32_t* withheld, relmc_hl1_seq_acc* acc,
                            relmc_hl1_seq_year* years_host);

/* ---- planned maintenance on the HL1 sequential chronology: up to 8 schedules against one fleet history (an extension beyond the reference) ---- */
/* What a maintenance plan costs in LOLE, EUE and LOLF, and whether plan B is better than plan A: up to 8 schedules are compared in ONE walk
 * of every chain, so their differences are paired under one seed.
 * Chronology  relmc_hl1_seq's, word for word (model of relmc_hl1_seq_load, draws (seed, chain, k | 0x40000000, event), both start rules,
 *             no FMA, DOWN on steps [ceil(T_odd), ceil(T_even))): under one seed, chain c of every schedule sees exactly the fleet history
 *             of chain c of relmc_hl1_seq.
 * Overlay     A unit's failure and repair process runs on regardless of maintenance; a unit on maintenance in an hour adds 0.0 to that
 *             hour's capacity (generating_adequancy_comparative.jl skips a unit in maintenance and samples the others by their FOR).
 *             Clocks that pause during maintenance are not modelled.
 * Windows     A schedule is a set of windows (unit, start_hour, hours) in hours of the year, 0-based, 0 <= start_hour < H,
 *             1 <= hours <= H, periodic in the year: unit k is on maintenance at hour-of-year h iff some window of k has
 *             (h - start_hour) mod H < hours.  A window that runs past the year's end therefore also covers the first hours of every year,
 *             chain year 0 included.  Windows of one unit may overlap (the union counts); a unit may have any number of windows, a
 *             schedule may have none.
 * Load        L(h) = scale * load[h] + shift, the product and the sum each rounded (relmc_hl1_seq_sweep's rule); one curve for the call,
 *             shared by all schedules.
 * Per step and schedule j: cap_j = sum over the units in ascending order of (UP and not on maintenance under j) ? cap_k : 0.0; loss iff
 *   cap_j < L(h) (strict), deficit L(h) - cap_j; per year and schedule: loss hours, EUE and loss events by relmc_hl1_seq's rules (step 1
 *   counts, an event across a year boundary counts once, in the year it starts; every schedule has its own previous-step flag).  A year's
 *   EUE is summed in relmc_hl1_seq's order (lane partials, then the fixed butterfly).
 * So (1) a schedule without windows gives, bit for bit, relmc_hl1_seq_sweep's level (scale, shift, fleet 0), and at (1.0, 0.0)
 *   relmc_hl1_seq's year records; (2) a schedule that keeps the units W on maintenance the whole year (start_hour 0, hours H) gives, bit
 *   for bit, the sweep's level (scale, shift, fleet 1) with withheld = W; (3) a schedule's year records depend on (seed, chain, start,
 *   years_per_chain, data, scale, shift, that schedule) only: not on the other schedules, their order, their number, or how a chain
 *   range is split into calls, and acc[j] is summed in a fixed order, so a repeated call is bitwise identical; (4) if schedule A's
 *   maintenance set contains schedule B's in every hour, every year's loss hours and EUE under A are >= those under B, exactly. */
#define RELMC_HL1_MAINT_MAX_SCHEDULES 8
typedef struct { int32_t schedule, unit, start_hour, hours; } relmc_hl1_maint_window;   /* 16 bytes */
/* The schedules of the next relmc_hl1_maint_seq calls, for the model relmc_hl1_seq_load has loaded (RELMC_ERR_NO_CASE before that call):
 * windows[i].schedule in 0 .. n_schedules - 1, unit in 0 .. ngen - 1, start_hour and hours as above.  The library keeps a per-schedule,
 * per-hour mask table on the device (four uint32 words per hour, bit k & 31 of word k >> 5 = unit k on maintenance: 16 bytes x nhours x
 * n_schedules) and the ngen and nhours it was built for.  RELMC_ERR_INVALID, with relmc_last_error naming the window and the field, for:
 * a null ctx; n_schedules outside 1 .. RELMC_HL1_MAINT_MAX_SCHEDULES; n_windows < 0; n_windows > 0 with windows == NULL; a window with
 * schedule, unit, start_hour or hours out of range.  A refused call changes nothing: the previous table still answers. */
int32_t relmc_hl1_maint_load(relmc_ctx* ctx, int32_t n_schedules, int64_t n_windows, const relmc_hl1_maint_window* windows);
/* chains [first_chain, first_chain + n_chains), each years_per_chain consecutive years, under every schedule of relmc_hl1_maint_load.
 * RELMC_ERR_NO_CASE before relmc_hl1_seq_load or relmc_hl1_maint_load.  RELMC_ERR_INVALID for: a null ctx or acc; a model of
 * relmc_hl1_seq_load whose ngen or nhours are not those the table was built for (load the schedules again after loading another model);
 * a non-finite scale or shift; anything relmc_hl1_seq refuses.  n_chains == 0 zeroes the outputs.
 *   acc         [n_schedules]
 *   years_host  optional [n_schedules][n_chains * years_per_chain], schedule-major, then chain-major
 * Long chain ranges go in launches of at most ~4M year records counted over all schedules; relmc_last_kernel_ms covers every launch. */
int32_t relmc_hl1_maint_seq(relmc_ctx* ctx, uint64_t seed, uint64_t first_chain, int64_t n_chains, int32_t years_per_chain,
                            int32_t start, double scale, double shift, relmc_hl1_seq_acc* acc,
                            relmc_hl1_seq_year* years_host);

/* ---- loss attribution on the HL1 sequential chronology: which units are down when load is lost (nsqMain.m:366-376, seqMain.m:144-158,233) ---- */
/* The reference ranks components by the share of its loss hours in which each was out (comp_importance).  Here every loss step of a chain
 * is charged to the units that are DOWN in it, and two of the charged quantities are exact counterfactuals on the same fleet history:
 * the units are independent, so a history with unit k always UP is this history with cap_k added wherever k is DOWN.
 * Chronology  relmc_hl1_seq's, word for word (model of relmc_hl1_seq_load, draws (seed, chain, k | 0x40000000, event), both start rules,
 *             no FMA, DOWN on steps [ceil(T_odd), ceil(T_even))): under one seed, chain c sees exactly the fleet history of chain c of
 *             relmc_hl1_seq.
 * Load        L = scale * load[h] + shift, the product and the sum each rounded (relmc_hl1_seq_sweep's rule).
 * Loss        iff cap_avail < L (strict), cap_avail the sum of the UP units' capacities in ascending unit order; deficit d = L - cap_avail.
 * Year records are bitwise relmc_hl1_seq_sweep's level (scale, shift, fleet 0), and at (1.0, 0.0) bitwise relmc_hl1_seq's; acc sums them
 *             as those calls do, launch by launch, so it is bitwise theirs whenever both calls take one launch (the chunk rule below).
 * Unit record of a chain, over all its steps n = 1 .. Y*H that are loss steps with unit k DOWN:
 *   down_hours      the number of such steps
 *   down_mwh        the sum of d
 *   critical_hours  the number of those with !(cap_avail + cap_k < L), the sum rounded once: the steps that would be no loss steps with k
 *                   UP (a tie cap_avail + cap_k == L counts).  Summed over a run, loss hours - critical_hours_k is the loss hours of the
 *                   fleet with unit k perfectly reliable, on the same history
 *   relief_mwh      the sum of fmin(d, cap_k): EUE - relief_mwh_k is that fleet's EUE
 *   The two fp64 sums are one accumulator per unit, added in ascending step order over the whole chain; the counts are exact (fp64,
 *   below 2^53).  Steps past Y*H do not exist.
 * unit_acc[k] sums x and x * x over the chains of the call, x = the chain's record of unit k in the field order above, reduced on the
 * device in a fixed order: a repeated call is bitwise equal.  A chain's own record depends on (seed, chain, start, years_per_chain,
 * data, scale, shift) only, never on the launch or call it is in. */
typedef struct { double down_hours, down_mwh, critical_hours, relief_mwh; } relmc_hl1_attr_unit;   /* 32 bytes */
typedef struct { double sum[4], sum2[4]; } relmc_hl1_attr_acc;                                     /* 64 bytes */
/* chains [first_chain, first_chain + n_chains), each years_per_chain consecutive years, of the model loaded by relmc_hl1_seq_load
 * (RELMC_ERR_NO_CASE before that call).  RELMC_ERR_INVALID for: a null ctx, acc or unit_acc; a non-finite scale or shift; anything
 * relmc_hl1_seq refuses.  A refused call changes nothing; n_chains == 0 zeroes the outputs.
 *   unit_acc    [ngen]
 *   years_host  optional [n_chains * years_per_chain], chain-major
 *   unit_host   optional [n_chains][ngen], chain-major
 * Long chain ranges go in launches of at most ~4M records, a chain counting years_per_chain + (4 * ngen + 2) / 3 (its year records and
 * its unit records in year records' size); relmc_last_kernel_ms covers every launch. */
int32_t relmc_hl1_attr_seq(relmc_ctx* ctx, uint64_t seed, uint64_t first_chain, int64_t n_chains, int32_t years_per_chain,
                           int32_t start, double scale, double shift, relmc_hl1_seq_acc* acc,
                           relmc_hl1_seq_year* years_host, relmc_hl1_attr_acc* unit_acc,
                           relmc_hl1_attr_unit* unit_host);

/* ---- energy storage on the HL1 sequential chronology: state of charge carried from hour to hour (an extension beyond the reference) ---- */
/* What a battery does to LOLE, EUE and LOLF exists only on a chronology: its state of charge couples the hours.  Up to 8 storages, given
 * in the call (as the sweep's levels are: no load call, no model state in the context), discharge into a shortfall of the fleet of
 * relmc_hl1_seq_load and charge from its surplus generation only.  Storages never fail.
 * Chronology  relmc_hl1_seq's, word for word (model of relmc_hl1_seq_load, draws (seed, chain, k | 0x40000000, event), start rules, no FMA,
 *             DOWN on steps [ceil(T_odd), ceil(T_even)), cap = sum over the UP units in ascending order): under one seed, chain c sees
 *             exactly the fleet history of chain c of relmc_hl1_seq.
 * Load        L(h) = scale * load[h] + shift, the product and the sum each rounded (relmc_hl1_seq_sweep's rule).
 * State       storage i has a state of charge s_i in MWh: soc0_mwh before step 1 of every chain, carried from step to step and from year
 *             to year inside a chain.
 * Arithmetic  every operation below is a separate, correctly rounded fp64 operation (no contraction, no FMA); min / max of two numbers.
 * Short step, cap < L:   need = L - cap; for i ascending while need > 0:
 *                            avail = min(discharge_mw_i, s_i * eta_discharge_i), x = min(avail, need),
 *                            s_i = max(0, s_i - x / eta_discharge_i), need = need - x.
 *                        The step is a loss step iff need > 0 afterwards, with deficit need; with need == 0 afterwards it counts in
 *                        served_hours.  The sum of the x (i ascending) goes to discharged_mwh.
 * Long step, cap > L:    surplus = cap - L; for i ascending while surplus > 0:
 *                            room = (energy_mwh_i - s_i) / eta_charge_i, y = min(min(charge_mw_i, room), surplus),
 *                            s_i = min(energy_mwh_i, s_i + y * eta_charge_i), surplus = surplus - y.
 *                        The sum of the y (i ascending) goes to charged_mwh.  A step with cap == L does nothing.
 * Year records  loss hours, EUE and loss events of the steps left after storage by relmc_hl1_seq's rules (step 1 counts, an event across a
 *             year boundary counts once, in the year it starts); the EUE of a year is summed in relmc_hl1_seq's order (the lanes'
 *             partials, then the fixed butterfly).  served_hours, discharged_mwh and charged_mwh of a year are summed over its steps in
 *             that same fixed order.
 * Consequences
 *   - With n_storage == 0 the year records are bitwise those of relmc_hl1_seq_sweep's level (scale, shift, fleet 0), and so are they when
 *     every storage has discharge_mw == 0, or energy_mwh == 0, or soc0_mwh == 0 together with charge_mw == 0; at (1.0, 0.0) they are
 *     bitwise relmc_hl1_seq's.  The storage records are then all zero.
 *   - served_hours + lole of a year equals that no-storage run's lole of the year exactly.
 *   - The storages deliver at most sum of discharge_mw in any hour, so for LOLE and EUE the risk with storage at load L + x is at least the
 *     no-storage risk at L once x >= sum of discharge_mw: the ELCC of a set of storages lies in [0, sum of discharge_mw]. */
#define RELMC_HL1_MAX_STORAGE 8
typedef struct { double charge_mw, discharge_mw, energy_mwh, eta_charge, eta_discharge, soc0_mwh; } relmc_hl1_storage;          /* 48 bytes */
typedef struct { double served_hours, discharged_mwh, charged_mwh; } relmc_hl1_storage_year;   /* short hours fully served, MWh delivered, MWh of surplus taken */
typedef struct {
    int64_t years;                                                          /* simulated years summed */
    double sum_lole, sum_eue, sum_lolf, sum_lole2, sum_eue2, sum_lolf2;
    double sum_served, sum_discharged, sum_charged, sum_served2, sum_discharged2, sum_charged2;
} relmc_hl1_storage_acc;
/* chains [first_chain, first_chain + n_chains), each years_per_chain consecutive years, of the model loaded by relmc_hl1_seq_load
 * (RELMC_ERR_NO_CASE before that call).  RELMC_ERR_INVALID, with relmc_last_error naming the storage and the field, for: a null ctx or
 * acc; n_storage outside 0 .. RELMC_HL1_MAX_STORAGE; n_storage > 0 with storage == NULL; a non-finite scale, shift or storage field; a
 * negative charge_mw, discharge_mw or energy_mwh; an efficiency outside (0, 1]; soc0_mwh outside [0, energy_mwh]; anything relmc_hl1_seq
 * refuses.  A refused call changes nothing; n_chains == 0 zeroes the outputs.
 *   storage             [n_storage], taken in this order at every step
 *   years_host          optional [n_chains * years_per_chain], chain-major
 *   storage_years_host  optional [n_chains * years_per_chain], chain-major
 * Results depend on (seed, chain, start, years_per_chain, data, scale, shift, storage) only, not on how a chain range is split into
 * calls; the sums of `acc` are taken in a fixed order, so a repeated call is bitwise identical.  Long chain ranges go in launches of at
 * most ~4M year records counted over both record rows, as in relmc_hl1_seq; relmc_last_kernel_ms covers every launch. */
int32_t relmc_hl1_seq_storage(relmc_ctx* ctx, uint64_t seed, uint64_t first_chain, int64_t n_chains, int32_t years_per_chain,
                              int32_t start, double scale, double shift, int32_t n_storage, const relmc_hl1_storage* storage,
                              relmc_hl1_storage_acc* acc, relmc_hl1_seq_year* years_host,
                              relmc_hl1_storage_year* storage_years_host);

/* ---- weather-year wind and solar resources on the HL1 sequential chronology, with storage (an extension beyond the reference) ---- */
/* Wind and solar are not Markov units: their output is an hourly profile that differs from weather year to weather year and is correlated
 * with the load of the same weather year.  A weather library holds n_weather such years, each with the hourly output of up to 8 resources
 * and, optionally, its own load curve; every chain year of a run draws one weather year, the fleet of relmc_hl1_seq_load fails and
 * repairs as ever, and the storages of relmc_hl1_seq_storage charge from the surplus that now includes the resources' output.  The
 * resources themselves never fail.
 * Chronology   relmc_hl1_seq's, word for word (model of relmc_hl1_seq_load, draws (seed, chain, k | 0x40000000, event), start rules, no FMA,
 *              DOWN on steps [ceil(T_odd), ceil(T_even))): under one seed, chain c sees exactly the fleet history of chain c of relmc_hl1_seq.
 * Weather year of chain year y (0-based) of chain c, w in 0 .. n_weather - 1:
 *              RELMC_HL1_VAR_PICK_RANDOM  w = ((uint64)x * n_weather) >> 32, x = word 0 of philox4x32_10(ctr = (c_lo, c_hi,
 *                                         RELMC_HL1_VAR_TAG, y), key = (seed_lo, seed_hi)): integer arithmetic, exact on every host
 *              RELMC_HL1_VAR_PICK_CYCLE   w = (c * years_per_chain + y) mod n_weather in unsigned 64-bit arithmetic
 *              w depends on nothing else, so not on how a chain range is split into calls.
 * Load         base(w, h) = load_mw[w][h] when the library has load curves, else relmc_hl1_seq_load's load[h];
 *              L = scale * base + shift, the product and the sum each rounded (relmc_hl1_seq_sweep's rule).
 * Capacity     cap = sum over the UP units in ascending order, as everywhere; then for r = 0 .. n_resources - 1 ascending
 *              cap = cap + resource_scale[r] * output_mw[w][r][h], the product and the sum each rounded (no contraction).  A scale of 0
 *              withholds a resource: it adds + 0.0, which is exact.
 * Storages     relmc_hl1_seq_storage's step rule, verbatim, with this cap and this L: the storages charge from the surplus, which includes
 *              the resources' output.  The state of charge is carried over the year boundary; the next year may be another weather year.
 * Year records, acc, the split and repeat guarantees and the launch chunk rule are relmc_hl1_seq_storage's (two record rows; a chain
 *              counts 2 * years_per_chain records).
 * Consequences
 *   1. With n_resources == 0 or every resource_scale == 0, and no load curves in the library, both record rows are bitwise those of
 *      relmc_hl1_seq_storage at (scale, shift, storages), under either pick; with n_storage == 0 and (1.0, 0.0) in addition they are
 *      bitwise relmc_hl1_seq's.
 *   2. With n_weather == 1, load curve X and no effective resource, the records are bitwise relmc_hl1_seq_storage's on the model loaded
 *      with X.
 *   3. When capacities, loads and outputs are all multiples of 2^-k of moderate size, so that every sum is exact, one resource with the
 *      constant output p gives bitwise the records of relmc_hl1_seq_sweep's level (scale, shift - p, fleet 0).
 *   4. Without storage, the sampled LOLE and EUE are non-increasing in every resource_scale[r] and non-decreasing in shift, chain by
 *      chain: the fleet history and the weather years are the same. */
#define RELMC_HL1_VAR_MAX_RESOURCES 8
#define RELMC_HL1_VAR_MAX_WEATHER   256
#define RELMC_HL1_VAR_TAG           0x60000000u   /* counter word 2 of a weather draw; 0x80000000, 0x40000000, 0x50000000, 0x20000000 are the other streams' */
#define RELMC_HL1_VAR_PICK_RANDOM   0
#define RELMC_HL1_VAR_PICK_CYCLE    1
/* The weather library: n_weather in 1 .. RELMC_HL1_VAR_MAX_WEATHER, n_resources in 0 .. RELMC_HL1_VAR_MAX_RESOURCES, nhours >= 1.  It
 * lives in a slot of its own: no other load call disturbs it, and it disturbs none.
 *   output_mw  [n_weather][n_resources][nhours], finite and >= 0; may be NULL iff n_resources == 0
 *   load_mw    optional [n_weather][nhours], finite: the load curve of each weather year
 * RELMC_ERR_INVALID, with relmc_last_error naming the weather year, the resource and the hour of the first bad value, for a value out of
 * these rules; RELMC_ERR_UNSUPPORTED for n_weather * max(n_resources, 1) * nhours >= 2^31 (the kernel indexes the library in 32 bits).
 * A refused call changes nothing. */
int32_t relmc_hl1_var_load(relmc_ctx* ctx, int32_t n_weather, int32_t n_resources, int32_t nhours,
                           const double* output_mw, const double* load_mw);
/* resource_scale: finite and >= 0, entries at or above n_resources must be 0; pick: RELMC_HL1_VAR_PICK_* */
typedef struct { double resource_scale[RELMC_HL1_VAR_MAX_RESOURCES]; double scale, shift; int32_t pick, reserved; } relmc_hl1_var_opts;  /* 88 bytes, reserved = 0 */
/* chains [first_chain, first_chain + n_chains), each years_per_chain consecutive years, of the fleet loaded by relmc_hl1_seq_load against
 * the weather loaded by relmc_hl1_var_load (RELMC_ERR_NO_CASE before either call; RELMC_ERR_INVALID, with a message that gives both
 * values, when their nhours differ).  RELMC_ERR_INVALID, with relmc_last_error naming the field, for: anything relmc_hl1_seq_storage
 * refuses; a null opts; a non-finite or negative resource_scale; a non-zero resource_scale at or above n_resources; pick not 0 or 1;
 * reserved != 0.  A refused call changes nothing; n_chains == 0 zeroes the outputs.
 *   years_host, storage_years_host  optional [n_chains * years_per_chain], chain-major
 *   weather_host                    optional [n_chains * years_per_chain], chain-major: the weather year of every chain year */
int32_t relmc_hl1_var_seq(relmc_ctx* ctx, uint64_t seed, uint64_t first_chain, int64_t n_chains, int32_t years_per_chain,
                          int32_t start, const relmc_hl1_var_opts* opts, int32_t n_storage, const relmc_hl1_storage* storage,
                          relmc_hl1_storage_acc* acc, relmc_hl1_seq_year* years_host,
                          relmc_hl1_storage_year* storage_years_host, int32_t* weather_host);
/* Host only, touches no device: the weather year of chain year `year` (0-based) of chain `chain`, or -1 for year < 0,
 * years_per_chain < 1, n_weather outside 1 .. RELMC_HL1_VAR_MAX_WEATHER or pick not 0 or 1. */
int32_t relmc_hl1_var_weather_year(uint64_t seed, uint64_t chain, int32_t year, int32_t years_per_chain, int32_t n_weather,
                                   int32_t pick);

/* ---- weather-dependent forced outage rates on that chronology: a stress library beside the weather library (an extension beyond the reference) ---- */
/* Thermal units fail more often in the cold snap or heat wave that also drives the peak load.  A stress library goes with the weather
 * library of relmc_hl1_var_load: for every weather year w, outage class c (at most RELMC_HL1_STRESS_MAX_CLASSES: gas, coal, nuclear ...)
 * and hour h a failure-rate multiplier fail_mult[w][c][h], finite and >= 0.  Every unit k of the relmc_hl1_seq_load fleet has a class
 * unit_class[k] in -1 .. n_classes - 1; a unit of class -1 ignores the weather.  A UP unit of class c fails with the hazard
 * fail_mult[w(y)][c][h] / mttf_k in hour h of chain year y, w(y) being relmc_hl1_var_weather_year's.  Repairs are unchanged: -mttr * ln U.
 * Cumulative table  per (w, c): G[0] = 0, G[j + 1] = G[j] + fail_mult[w][c][j], one rounded addition per hour, H + 1 values
 *              (relmc_hl1_stress_cumulative).  Only G goes to the device, and the contract is stated on G alone: the hazard consumed within
 *              hour j is the linear interpolation of G[j] .. G[j + 1].
 * Failure time  a unit becomes UP at chain time T (or is UP at the start, T = 0).  The draw and the product are relmc_hl1_seq's:
 *              E = -mttf * ln U rounded once, U the draw (seed, chain, k | 0x40000000, event).  Class -1: the next transition is T + E.
 *              Otherwise (relmc_hl1_stress_failure_time), every operation a separate rounded fp64 operation, no contraction, with
 *              H = nhours, Y = years_per_chain and G the row of (w(y), c):
 *                0. if not T < Y * H (UP again at or after the chain's end): the result is max(T, Y * H + 1)
 *                1. n0 = floor(T), y = n0 div H, j = n0 mod H in integers, frac = T - n0
 *                2. a = G[j] + (G[j + 1] - G[j]) * frac;  rem = G[H] - a
 *                3. while E > rem (strict): E = E - rem, y = y + 1; if y == Y the result is Y * H + 1 (the unit does not fail within
 *                   the chain); else j = 0, a = 0, rem = G[H] of the new year's row
 *                4. t = a + E;  j' = the smallest index in j .. H - 1 with G[j' + 1] >= t, H - 1 if rounding leaves none
 *                5. d = G[j' + 1] - G[j'];  frac' = d > 0 ? (t - G[j']) / d : 1, clamped to [0, 1]
 *                6. the result is max(T, (y * H + j') + frac')
 * Everything else is relmc_hl1_var_seq's, word for word: DOWN on steps [ceil(T_odd), ceil(T_even)), the resources, the load rule, the
 *              storages, the two record rows, the start rules, the launch chunk rule, the split and repeat guarantees.
 *              RELMC_HL1_START_STATIONARY keeps the base q = mttr / (mttf + mttr) for draw 0: under a varying multiplier the process is
 *              NOT stationary, and that start is then only a start closer to the long-run mix than all-UP.
 * Consequences
 *   1. With every unit in class -1, both record rows are bitwise relmc_hl1_var_seq's, under either pick and with any storages.
 *   2. With years_per_chain == 1 and the all-UP start, a multiplier of 1.0 in every hour gives bitwise relmc_hl1_var_seq's records, and
 *      a multiplier of exactly 2.0 in every hour for the units of one class gives bitwise the records of relmc_hl1_var_seq on the fleet
 *      with those units' mttf halved (G, 2T and E / 2 are exact then; a draw that ends within rounding of the year's end apart).
 *   3. With years_per_chain > 1 and multiplier 1.0 a unit's position within the year, not its chain time, enters the sum, so transition
 *      times may differ from relmc_hl1_var_seq's in the last bit; the steps they take effect on differ only when a time lies within
 *      rounding of an integer.  No bitwise guarantee is given; the tests hold the per-year integers equal on their chains.
 *   4. A weather year whose multipliers are all 0 for a class is passed with E unchanged: a unit of that class cannot fail in it.
 *   5. Under one seed, units of class -1 have exactly the history they have in relmc_hl1_var_seq. */
#define RELMC_HL1_STRESS_MAX_CLASSES 8
/* The stress library: n_weather in 1 .. RELMC_HL1_VAR_MAX_WEATHER, n_classes in 1 .. RELMC_HL1_STRESS_MAX_CLASSES, nhours >= 1, n_units in
 * 1 .. 128.  It builds G and uploads it; it lives in a slot of its own: no other load call disturbs it, and it disturbs none.
 *   fail_mult   [n_weather][n_classes][nhours], finite and >= 0
 *   unit_class  [n_units], -1 .. n_classes - 1
 * RELMC_ERR_INVALID, with relmc_last_error naming the weather year, the class and the hour of the first non-finite or negative
 * multiplier, or the unit with a class out of range; RELMC_ERR_UNSUPPORTED for n_weather * n_classes * (nhours + 1) >= 2^31 (the kernel
 * indexes the tables in 32 bits).  A refused call changes nothing. */
int32_t relmc_hl1_stress_load(relmc_ctx* ctx, int32_t n_weather, int32_t n_classes, int32_t nhours, const double* fail_mult,
                              int32_t n_units, const int32_t* unit_class);
/* relmc_hl1_var_seq's argument list and outputs, with the failure rule above.  RELMC_ERR_NO_CASE before any of relmc_hl1_seq_load,
 * relmc_hl1_var_load and relmc_hl1_stress_load; RELMC_ERR_INVALID, with both values in the message, when n_units differs from the
 * fleet's or n_weather or nhours differ from relmc_hl1_var_load's; everything relmc_hl1_var_seq refuses is refused here too.  A refused
 * call changes nothing; n_chains == 0 zeroes the outputs. */
int32_t relmc_hl1_stress_seq(relmc_ctx* ctx, uint64_t seed, uint64_t first_chain, int64_t n_chains, int32_t years_per_chain,
                             int32_t start, const relmc_hl1_var_opts* opts, int32_t n_storage, const relmc_hl1_storage* storage,
                             relmc_hl1_storage_acc* acc, relmc_hl1_seq_year* years_host,
                             relmc_hl1_storage_year* storage_years_host, int32_t* weather_host);
/* Host only, touches no device: cum_out[0 .. nhours] = the cumulative table G of one row of multipliers.  RELMC_ERR_INVALID for
 * nhours < 1, a null pointer or a multiplier that is not finite and >= 0. */
int32_t relmc_hl1_stress_cumulative(int32_t nhours, const double* fail_mult_row, double* cum_out);
/* Host only, touches no device: the failure time above for one draw, compiled from the text the kernel is compiled from.
 *   t, e     the time the unit became UP (finite, >= 0) and the draw -mttf * ln U (>= 0)
 *   weather  [years_per_chain]: the weather year of every chain year, each in 0 .. RELMC_HL1_VAR_MAX_WEATHER - 1
 *   cum      [n_weather][nhours + 1]: the cumulative tables of ONE class, n_weather above every entry of `weather`
 * NaN for an argument out of these rules. */
double relmc_hl1_stress_failure_time(double t, double e, int32_t nhours, int32_t years_per_chain, const int32_t* weather,
                                     const double* cum);

/* ---- HL1 sequential chronology with derated states: three-state Markov units (an extension beyond the reference) ---- */
/* A large thermal unit that loses a feed pump or a mill runs at part load for days: the textbook third state (Billinton & Allan), with
 * its own capacity and transition rates.  The reference's units, and every other HL1 track here, are two-state.
 * States      0 = UP at capacity_mw, 1 = DERATED at derated_mw (0 <= derated_mw <= capacity_mw), 2 = DOWN at 0.
 * Unit        a continuous-time Markov chain, given per state i by mean_h[i], the mean holding time in hours, and first_p[i], the
 *             probability that the sojourn ends in the FIRST-LISTED destination:
 *                 from UP: (DOWN, DERATED)      from DERATED: (UP, DOWN)      from DOWN: (UP, DERATED)
 *             A two-state unit is mean_h = (mttf, any, mttr), first_p = (1, any, 1).  Means and branch probabilities, not a rate matrix,
 *             are the ABI form: only so is the two-state case bitwise relmc_hl1_seq's (-mttf * ln U with the caller's own mttf).
 * Chronology  relmc_hl1_seq's (steps n = 1 .. Y*H, state carried from year to year), extended.  With T_1 < T_2 < ... a unit's transition
 *             times and T_0 = 0, the sojourn that starts at T_j covers steps ceil(T_j) .. ceil(T_j+1) - 1 (none when both ends round up to
 *             the same step).  T_j+1 = T_j + (-mean_h[state] * ln U), the product and the sum each rounded (no FMA); duration draw e of
 *             unit k is relmc_hl1_seq's draw e: (seed, chain, k | 0x40000000, e), the same stream and numbering.
 * Branches    the destination of the transition that ends the sojourn timed by duration draw e is taken from draw e of a second stream,
 *             (seed, chain, k | RELMC_HL1_MS_BRANCH_TAG, e), formed as the duration draws are: the first-listed destination iff
 *             U < first_p[state].  With first_p exactly 1 or 0 the draw cannot matter (and is not generated).
 * Start       RELMC_HL1_START_ALL_UP as relmc_hl1_seq.  RELMC_HL1_START_STATIONARY: draw 0 picks the state from the stationary law pi,
 *             DOWN iff U < pi_2, else DERATED iff U < pi_2 + pi_1, else UP; durations from draw 1 on.  pi_i is proportional to
 *             nu_i * mean_h[i] with nu the stationary vector of the embedded jump chain over the states reachable from UP,
 *                 nu_0 = f_2 + f_1 (1 - f_2),  nu_1 = (1 - f_2) + f_2 (1 - f_0),  nu_2 = (1 - f_1) + f_1 f_0      (f = first_p),
 *                 w_i = nu_i * mean_h[i],  pi_2 = w_2 / ((w_0 + w_1) + w_2),  pi_1 = w_1 / ((w_0 + w_1) + w_2);
 *             a unit that never reaches DERATED has pi_1 = 0 and pi_2 = mean_h[2] / (mean_h[0] + mean_h[2]), relmc_hl1_seq_load's own
 *             expression, and one that never reaches DOWN pi_2 = 0 and pi_1 = mean_h[1] / (mean_h[0] + mean_h[1]).
 * Per step    cap_avail summed in ascending unit order: capacity_mw for UP, derated_mw for DERATED, 0.0 for DOWN; loss iff
 *             cap_avail < load (strict); events, year attribution and the EUE summation order are relmc_hl1_seq's.  A year's second
 *             record counts its (unit, step) pairs DERATED and DOWN.
 * The pin     a model whose units all have first_p[0] == first_p[2] == 1 gives year records that are bitwise relmc_hl1_seq's on the
 *             relmc_hl1_seq_load model (capacity_mw, mean_h[0], mean_h[2]), under both start rules. */
#define RELMC_HL1_MS_MAX_HOURS 1073741824      /* 2^30: the longest load curve relmc_hl1_ms_load takes */
#define RELMC_HL1_MS_BRANCH_TAG 0x50000000u   /* counter word 2 of a branch draw is k | this; 0x80000000, 0x40000000, 0x20000000 are the other streams' */
typedef struct { double capacity_mw, derated_mw, mean_h[3], first_p[3]; } relmc_hl1_ms_unit;          /* 64 bytes */
typedef struct { double derated_unit_h, down_unit_h; } relmc_hl1_ms_year;      /* unit-hours of one simulated year spent DERATED / DOWN, over the fleet */
typedef struct {
    int64_t years;                                                          /* simulated years summed */
    double sum_lole, sum_eue, sum_lolf, sum_lole2, sum_eue2, sum_lolf2;
    double sum_derated, sum_down, sum_derated2, sum_down2;
} relmc_hl1_ms_acc;
/* Fleet (ngen <= 128 units) and the hourly load curve of one year (nhours >= 1).  The model lives in a slot of its own: relmc_hl1_load,
 * relmc_hl1_seq_load, relmc_hl1_plan_load and relmc_hl1_area_load do not disturb it, and it does not disturb them.
 * RELMC_ERR_INVALID, with relmc_last_error naming the unit (and the state) or the hour, for: what the input rule of the four HL1 load
 * calls refuses; a non-finite field; derated_mw outside [0, capacity_mw]; a first_p outside [0, 1] or a mean_h <= 0 of a state that can be
 * reached from UP; a chain in which some state reachable from UP cannot return to UP (the stationary law is then not unique).  A state that
 * cannot be reached from UP is ignored entirely: its fields need only be finite.  RELMC_ERR_UNSUPPORTED for more than 128 units or more than
 * RELMC_HL1_MS_MAX_HOURS hours (the kernel counts a lane's unit-hours of a year in 32 bits).  A refused call changes nothing. */
int32_t relmc_hl1_ms_load(relmc_ctx* ctx, int32_t ngen, const relmc_hl1_ms_unit* units, int32_t nhours, const double* load_mw);
/* chains [first_chain, first_chain + n_chains), each years_per_chain consecutive years, of the model loaded by relmc_hl1_ms_load
 * (RELMC_ERR_NO_CASE before that call); arguments are checked as relmc_hl1_seq checks them, a refused call changes nothing,
 * n_chains == 0 zeroes the outputs.
 *   years_host        optional [n_chains * years_per_chain], chain-major
 *   state_years_host  optional [n_chains * years_per_chain], chain-major
 * Results depend on (seed, chain, start, years_per_chain, data) only, not on how a chain range is split into calls; the sums of `acc`
 * are taken in a fixed order, so a repeated call is bitwise identical.  Long chain ranges go in launches of at most ~4M year records
 * counted over both record rows, as in relmc_hl1_seq_storage; relmc_last_kernel_ms covers every launch. */
int32_t relmc_hl1_ms_seq(relmc_ctx* ctx, uint64_t seed, uint64_t first_chain, int64_t n_chains, int32_t years_per_chain, int32_t start,
                         relmc_hl1_ms_acc* acc, relmc_hl1_seq_year* years_host, relmc_hl1_ms_year* state_years_host);

/* ---- HL1 multi-area chronology with tie-line transfers (AdequacyAssessmentII.jl:73-250 solve_curtailment_fast / run_fast_sequential_simulation) ---- */
/* The chronology is relmc_hl1_seq's, word for word: draws (seed, chain, k | 0x40000000, event) with k the GLOBAL unit index (units stored
 * area-major: area 0's units, then area 1's, ...), the same start rules, steps n = 1 .. Y*H with the state carried across years, no FMA.
 * A one-area run without ties therefore has relmc_hl1_seq's chronology, and ISOLATED / INTERCONNECTED runs of one seed see the same fleet.
 * Per step (every area shares nhours H, 0-based areas):
 *   m_i = cap_i - load_i[h], cap_i = sum of area i's UP units' capacities in ascending unit order.
 *   T[i][j] = T[j][i] = sum of the capacities of the ties between i and j (parallel ties summed in tie order; a tie fails only with
 *     relmc_hl1_area_tie_outages' data, below).
 *   every m_i >= 0: nothing is curtailed.  ISOLATED: no transfer.
 *   INTERCONNECTED, RELMC_HL1_AREA_FLOW_REFERENCE (:105-167): R = T; loop { s = lowest i with m_i > 1e-4, t = lowest i with m_i < -1e-4,
 *     stop if either is missing; BFS from s (FIFO queue [s], s marked; pop u, u == t: path found; else for v = 0..n-1 ascending, if
 *     R[u][v] > 1e-4 and v unmarked: parent[v] = u, mark v, push v); no path: STOP the whole loop (the reference's break);
 *     f = min(m_s, -m_t), then f = min(f, R[parent[v]][v]) along the path; m_s -= f; m_t += f; R[p][v] -= f, R[v][p] += f on the path }.
 *   INTERCONNECTED, RELMC_HL1_AREA_FLOW_MAX_FLOW: the same BFS from each source s (m_s > 1e-4) in ascending order, ending at the first
 *     popped area u with m_u < -1e-4 (the sink); augment as above and restart from the lowest source; stop when no source reaches a
 *     deficit: a maximum flow of the super-source / super-sink graph, so the total curtailment is the least possible.
 *   Both rules stop after at most 4096 augmentations per step (a guard; not reached on 8 areas).
 *   c_i = -m_i if m_i < 0 else 0; area i has a loss hour iff c_i > 0; the system has one iff any c_i > 0, its deficit sum c_i in area order.
 * Per year, for each area and for the system: loss hours, EUE and loss events (rising edges of the flag along the chain, step 1 counts,
 * an event counts in the year it starts), as relmc_hl1_seq. */
#define RELMC_AREA_MAX 8
#define RELMC_HL1_AREA_ISOLATED        0
#define RELMC_HL1_AREA_INTERCONNECTED  1
#define RELMC_HL1_AREA_FLOW_REFERENCE  0
#define RELMC_HL1_AREA_FLOW_MAX_FLOW   1
/* n_areas <= RELMC_AREA_MAX areas of units_per_area[i] >= 1 units each (<= 128 units in total; capacity_mw / mttf_h / mttr_h area-major,
 * mttf / mttr finite and > 0), hourly_load_mw [n_areas][nhours], n_ties >= 0 ties (0-based endpoints in range, from != to, capacity
 * finite and >= 0).  Held apart from the relmc_hl1_load / relmc_hl1_seq_load / relmc_hl1_plan_load models: no call disturbs another. */
int32_t relmc_hl1_area_load(relmc_ctx* ctx, int32_t n_areas, const int32_t* units_per_area, const double* capacity_mw,
                            const double* mttf_h, const double* mttr_h, int32_t nhours, const double* hourly_load_mw,
                            int32_t n_ties, const int32_t* tie_from, const int32_t* tie_to, const double* tie_capacity_mw);
/* chains [first_chain, first_chain + n_chains) of years_per_chain years; policy RELMC_HL1_AREA_*, flow RELMC_HL1_AREA_FLOW_* (read under
 * INTERCONNECTED only, but always checked).  acc: [n_areas + 1], row n_areas = the system.  years_host: optional
 * [n_chains * years_per_chain][n_areas + 1], chain-major.  Results depend on (seed, chain, start, years_per_chain, policy, flow, data)
 * only, not on how a chain range is split into calls; sums are taken in a fixed order, so a repeated call is bitwise identical. */
int32_t relmc_hl1_area(relmc_ctx* ctx, uint64_t seed, uint64_t first_chain, int64_t n_chains, int32_t years_per_chain, int32_t start,
                       int32_t policy, int32_t flow, relmc_hl1_seq_acc* acc, relmc_hl1_seq_year* years_host);
/* Tie outages (an extension: the reference's ties never fail).  Tie t (0-based, in relmc_hl1_area_load's order) is a two-state component
 * with tie_mttf_h[t] / tie_mttr_h[t] hours.  Its chronology is relmc_hl1_seq's, word for word (draws, -m ln U in fp64, product and sum each
 * rounded, DOWN on steps [ceil(T_odd), ceil(T_even)), both start rules with DOWN iff U < mttr / (mttf + mttr) under STATIONARY), with
 * component index k = RELMC_HL1_TIE_DRAW_BASE + t in the counter word ((128 + t) | 0x40000000).  Units use k < 128, so the fleet's history
 * does not depend on whether ties fail: runs with and without tie outages under one seed see the same unit states.
 *   tie_mttf_h[t] = +INFINITY: tie t never fails; it takes no draws and tie_mttr_h[t] is not read.  Every other mttf, and its mttr, must be
 *   finite and > 0.
 *   Per step, T[i][j] = T[j][i] = the sum, from 0.0 in ascending tie order, of the capacities of the ties between i and j that are UP in
 *   that step (with every tie UP: the matrix relmc_hl1_area_load holds).  Everything after T is unchanged; ISOLATED never reads T.
 * At most RELMC_HL1_TIE_MAX ties when outage data is set.  RELMC_ERR_INVALID, with relmc_last_error naming the tie: more ties than that, a
 * count that differs from the loaded model's, a mttf that is NaN, <= 0 or -INFINITY, a mttr of a failing tie that is not finite and > 0.
 * A refused call changes nothing.  RELMC_ERR_NO_CASE before relmc_hl1_area_load. */
#define RELMC_HL1_TIE_MAX 32
#define RELMC_HL1_TIE_DRAW_BASE 128
/* Forced outages of the ties of the loaded multi-area model.  n_ties = the loaded count.  NULL, NULL (or n_ties = 0) removes
 * the outage data.  relmc_hl1_area_load removes it too.  Read by relmc_hl1_area under INTERCONNECTED; the split / repeat guarantees of
 * relmc_hl1_area hold with it as they are. */
int32_t relmc_hl1_area_tie_outages(relmc_ctx* ctx, int32_t n_ties, const double* tie_mttf_h, const double* tie_mttr_h);

/* ---- sweep of the multi-area chronology: one fleet and tie history against up to 8 levels of load, tie capacity and fleet (an extension) ---- */
/* How an area's risk falls as tie capacity is added, how much more load an area carries because it is interconnected, and what a unit is
 * worth once neighbours lean on it are each a curve of relmc_hl1_area results; this call gives up to 8 points of such a curve from ONE
 * walk of every chain.  It runs on the model of relmc_hl1_area_load, and on relmc_hl1_area_tie_outages' data when set: under one seed,
 * chain c of every level sees exactly the unit and tie history of chain c of relmc_hl1_area.  The policy is INTERCONNECTED.
 * Level j is the model it is equivalent to:
 *   load    of area a at hour h: load_scale[a] * load[a][h] + load_shift[a], the product and the sum each rounded (no FMA; numpy's
 *           scale * load + shift).  Entries at or above n_areas are not read.
 *   fleet   0: every unit; 1: every unit except those whose bit is set in `withheld` (bit k & 31 of word k >> 5, k the GLOBAL unit index):
 *           a withheld unit adds 0.0 in the same ascending loop (relmc_hl1_seq_sweep's rule and mask format).
 *   ties    the capacity of tie t is tie_scale * cap_t (rounded) where tie_scaled is NULL or tie_scaled[t] != 0, else cap_t.  T is formed
 *           from those capacities exactly as relmc_hl1_area forms it: parallel ties summed in tie order, only the UP ties on a step with a
 *           tie DOWN.
 *   Everything after T is relmc_hl1_area's: margins, the transfer solve, c_i, the flags, events, and the year's EUE in that kernel's order.
 * Two guarantees follow:
 *   1. Level j's year records are BITWISE those of relmc_hl1_area(INTERCONNECTED, flow) on the model loaded with level j's load curves
 *      (numpy's scale * load + shift), the scaled tie capacities, and the withheld units' capacities as 0.0.
 *   2. A level whose scaled ties all have tie_scale == 0 (tie_scaled == NULL: every tie) is bitwise RELMC_HL1_AREA_ISOLATED.
 * A level's year records depend on (seed, chain, start, years_per_chain, flow, data, that level, the two masks) only: not on the other
 * levels, their order, or how a chain range is split into calls.  acc is summed in a fixed order, so a repeated call is bitwise identical.
 * Only the system row under RELMC_HL1_AREA_FLOW_MAX_FLOW is monotone in load and in tie capacity, and only up to the solve's 1e-4
 * thresholds; an area's own row, and any row under FLOW_REFERENCE, need not be. */
#define RELMC_HL1_AREA_SWEEP_MAX_LEVELS (8)
typedef struct {
    double load_scale[RELMC_AREA_MAX], load_shift[RELMC_AREA_MAX];
    double tie_scale;
    int32_t fleet;
    int32_t reserved;
} relmc_hl1_area_level;   /* 144 bytes, reserved = 0 */
/* chains [first_chain, first_chain + n_chains), each years_per_chain consecutive years; flow RELMC_HL1_AREA_FLOW_*.
 *   withheld    optional [4] mask words (128 units)
 *   tie_scaled  optional [n_ties of relmc_hl1_area_load]
 *   acc         [n_levels][n_areas + 1], row n_areas = the system
 *   years_host  optional [n_levels][n_chains * years_per_chain][n_areas + 1], level-major, then chain-major
 * RELMC_ERR_INVALID, with relmc_last_error naming the level, area, bit or tie, for: a null levels or acc; n_levels outside
 * 1 .. RELMC_HL1_AREA_SWEEP_MAX_LEVELS; a non-finite scale or shift among the first n_areas entries; tie_scale not finite or below 0 (or a
 * scaled capacity that is not finite); fleet not 0 or 1; reserved != 0; fleet 1 with withheld == NULL; a withheld bit at or above ngen;
 * anything relmc_hl1_area refuses.  A refused call changes nothing; n_chains == 0 zeroes the outputs.  RELMC_ERR_NO_CASE before
 * relmc_hl1_area_load.  The call never changes the loaded model: a relmc_hl1_area run after it is bitwise what it was before.
 * Long chain ranges go in launches of at most ~4M year records counted over levels and rows; relmc_last_kernel_ms covers every launch. */
int32_t relmc_hl1_area_sweep(relmc_ctx* ctx, uint64_t seed, uint64_t first_chain, int64_t n_chains, int32_t years_per_chain,
                             int32_t start, int32_t flow, int32_t n_levels, const relmc_hl1_area_level* levels,
                             const uint32_t* withheld, const uint8_t* tie_scaled, relmc_hl1_seq_acc* acc,
                             relmc_hl1_seq_year* years_host);

/* ---- weather-year resources and storages in the areas of the multi-area chronology (an extension beyond the reference) ---- */
/* What wind, solar and a battery in area B are worth to B and to its neighbours across a limited tie exists only on the multi-area
 * chronology: subtracting a profile from an area's load by hand gives one weather year, no sampling and no storage.  A weather library
 * of the areas holds n_weather years, each with the hourly output of up to 8 resources, every one placed in an area, and, optionally, a
 * load curve of every area; up to 8 storages, each placed in an area, are given in the call.  Resources and storages never fail.
 * Per step, every operation is one correctly rounded fp64 operation (no contraction, no FMA):
 *   1. Chronology    relmc_hl1_area's, word for word: units are global component k < 128, ties component 128 + t, the same start rules.
 *                    Under one seed, chain c sees exactly the unit and tie history of chain c of relmc_hl1_area.
 *   2. Weather year  of chain year y: relmc_hl1_var_weather_year's function, verbatim, with the same tag RELMC_HL1_VAR_TAG.  A one-area
 *                    run therefore sees relmc_hl1_var_seq's weather.
 *   3. Load          L_a = load_scale[a] * base_a(w, h) + load_shift[a], the product and the sum each rounded; base_a(w, h) =
 *                    load_mw[w][a][h] when the library has load curves, else relmc_hl1_area_load's load[a][h].
 *   4. Capacity      cap_a = sum of area a's UP units in ascending order; then, for r ascending over the resources with
 *                    resource_area[r] == a, cap_a = cap_a + resource_scale[r] * output_mw[w][r][h], the product and the sum each rounded.
 *                    The margin is m_a = cap_a - L_a.
 *   5. Transfers first.  ISOLATED: none.  INTERCONNECTED: relmc_hl1_area's transfer solve on these margins, unchanged (both flow rules,
 *                    the 1e-4 thresholds, the 4096 guard, T from the UP ties), which leaves the post-transfer margins m'_a.
 *   6. Storage last, and local.  In every area a, its storages in array order apply relmc_hl1_seq_storage's step rule, verbatim:
 *                    m'_a < 0: need = -m'_a, the storages discharge while need is left; the area's deficit is what is left.
 *                    m'_a > 0: surplus = m'_a, the storages charge from it.          m'_a == 0: nothing happens.
 *                    A state of charge starts at soc0_mwh in every chain and is carried across steps and years.
 *      THE POLICY: energy-limited resources are used after the ties.  A storage neither exports nor charges from imports beyond what
 *                    step 5 left in its area; the transfer solve never sees a state of charge.  A pooled or export policy is not built.
 *   7. Flags and records.  Area a has a loss hour iff a deficit > 0 is left after step 6; the system has one iff any area has, its
 *                    deficit the sum in area order.  Loss hours, EUE and events of every row follow relmc_hl1_area's rules.  A second
 *                    record of every row is a relmc_hl1_storage_year: served_hours counts the steps on which the area was short after
 *                    step 5 and nothing is left after step 6 (the system: some area was short after step 5, none is after step 6);
 *                    discharged_mwh / charged_mwh are the step sums of x / y over the area's storages in order (the system: the areas'
 *                    step sums in area order).  A year's sums are taken in relmc_hl1_area's fixed order: lane partials, then the butterfly.
 * Consequences
 *   C1. No effective resource (none, or every scale 0), no curves in the library, no storage, load_scale 1 and load_shift 0: the loss
 *       records are bitwise relmc_hl1_area(policy, flow)'s, with and without tie-outage data; with other scales and shifts they are
 *       bitwise relmc_hl1_area's on the model loaded with the curves load_scale[a] * load_a[h] + load_shift[a].
 *   C2. One area, no ties: both records of area 0 and of the system are bitwise relmc_hl1_var_seq's two records with the same fleet,
 *       library, scales and storages at (scale, shift) = (load_scale[0], load_shift[0]), under both picks.
 *   C3. ISOLATED: area a's two records are bitwise relmc_hl1_var_seq's on the pooled fleet with the other areas' capacities at 0, area
 *       a's curve(s), the other areas' resources at scale 0 and only area a's storages, in order.  INTERCONNECTED with every tie
 *       capacity 0 is bitwise ISOLATED.
 *   C4. For every row and year, served_hours + lole equals the lole of the same call with n_storage == 0, exactly: storage comes after
 *       the transfers and never feeds back into them.
 *   C5. Storages that cannot act (discharge_mw == 0, or energy_mwh == 0, or soc0_mwh == 0 together with charge_mw == 0) give loss
 *       records bitwise those of n_storage == 0 and served_hours == discharged_mwh == 0.  charged_mwh is 0 as well, except that a
 *       storage with discharge_mw == 0 and room left still charges by the step rule (as in relmc_hl1_seq_storage) and never delivers.
 *   C6. On multiples of 2^-k of moderate size, so that every sum is exact, one resource in area a with the constant output p gives
 *       bitwise the records of the same call without it at load_shift[a] - p. */
/* The weather library of the areas: n_areas in 1 .. RELMC_AREA_MAX, n_weather in 1 .. RELMC_HL1_VAR_MAX_WEATHER, n_resources in
 * 0 .. RELMC_HL1_VAR_MAX_RESOURCES, nhours >= 1.  It lives in a slot of its own: no other load call disturbs it, and it disturbs none.
 *   resource_area  [n_resources], 0-based, in 0 .. n_areas - 1; may be NULL iff n_resources == 0
 *   output_mw      [n_weather][n_resources][nhours], finite and >= 0; may be NULL iff n_resources == 0
 *   load_mw        optional [n_weather][n_areas][nhours], finite: the load curve of every area in every weather year
 * RELMC_ERR_INVALID, with relmc_last_error naming the weather year, the resource or area, and the hour of the first bad value, for a value
 * out of these rules; RELMC_ERR_UNSUPPORTED for more than RELMC_AREA_MAX areas and for n_weather * max(n_resources, n_areas, 1) * nhours
 * >= 2^31 (the kernel indexes the library in 32 bits).  A refused call changes nothing. */
int32_t relmc_hl1_area_var_load(relmc_ctx* ctx, int32_t n_areas, int32_t n_weather, int32_t n_resources, const int32_t* resource_area,
                                int32_t nhours, const double* output_mw, const double* load_mw);
/* resource_scale: finite and >= 0, 0 at or above n_resources; load_scale / load_shift: finite, 1 / 0 at or above n_areas; policy
 * RELMC_HL1_AREA_*, flow RELMC_HL1_AREA_FLOW_* (read under INTERCONNECTED only, but always checked), pick RELMC_HL1_VAR_PICK_* */
typedef struct {
    double resource_scale[RELMC_HL1_VAR_MAX_RESOURCES];
    double load_scale[RELMC_AREA_MAX], load_shift[RELMC_AREA_MAX];
    int32_t policy, flow, pick, reserved;
} relmc_hl1_area_var_opts;   /* 208 bytes, reserved = 0 */
/* a storage of relmc_hl1_seq_storage (the same field rules) in the 0-based area `area` */
typedef struct { relmc_hl1_storage s; int32_t area, reserved; } relmc_hl1_area_storage;   /* 56 bytes, reserved = 0 */
/* chains [first_chain, first_chain + n_chains), each years_per_chain consecutive years, of the model of relmc_hl1_area_load, and of
 * relmc_hl1_area_tie_outages' data when set and the policy is INTERCONNECTED (exactly as relmc_hl1_area), against the library of
 * relmc_hl1_area_var_load.  RELMC_ERR_NO_CASE before either load call; RELMC_ERR_INVALID, with a message that gives both values, when
 * n_areas or nhours of the two differ or a resource_area is out of range for the model.  RELMC_ERR_INVALID, naming the storage and the
 * field, for: anything relmc_hl1_area refuses; a null opts; a scale or shift out of the rules above; policy, flow or pick not 0 or 1;
 * reserved != 0; n_storage outside 0 .. RELMC_HL1_MAX_STORAGE (all areas together); a storage's area out of range; anything
 * relmc_hl1_seq_storage refuses in a storage's fields.  A refused call changes nothing; n_chains == 0 zeroes the outputs.
 *   storage             [n_storage]; the storages of one area act in this array's order
 *   acc                 [n_areas + 1], row n_areas = the system
 *   years_host          optional [n_chains * years_per_chain][n_areas + 1], chain-major
 *   storage_years_host  optional [n_chains * years_per_chain][n_areas + 1], chain-major
 *   weather_host        optional [n_chains * years_per_chain], chain-major: the weather year of every chain year
 * The split and repeat guarantees are relmc_hl1_area's.  Long chain ranges go in launches of at most ~4M year records, a chain counting
 * 2 * (n_areas + 1) * years_per_chain; relmc_last_kernel_ms covers every launch. */
int32_t relmc_hl1_area_var(relmc_ctx* ctx, uint64_t seed, uint64_t first_chain, int64_t n_chains, int32_t years_per_chain,
                           int32_t start, const relmc_hl1_area_var_opts* opts, int32_t n_storage,
                           const relmc_hl1_area_storage* storage, relmc_hl1_storage_acc* acc, relmc_hl1_seq_year* years_host,
                           relmc_hl1_storage_year* storage_years_host, int32_t* weather_host);

/* ---- HL1 planning model: maintenance, energy-limited units, LFU(generating_adequancy_comparative.jl:15-120, tail_risk.jl:12-91) ---- */
/* Year y is the global index first_year + i; hour h is 0-based; every year starts with every ELU's energy at 0; years are independent.
 * Block b of hour h of year y: philox4x32_10(ctr = (y_lo, y_hi, 0x20000000 | h, b), key = (seed_lo, seed_hi)); word j = word j & 3 of
 * block j >> 2 (the 0x20000000 tag keeps these draws apart from the 0x40000000 / 0x80000000 chronologies and the non-sequential draws).
 *   LFU:   U_i = (word_i + 0.5) / 2^32 (i = 0, 1), z = sqrt(-2 ln U_1) * cos(2 pi U_2), load = load_h + z * sigma (product and sum each
 *          rounded, no FMA)
 *   units: unit k is in maintenance in week w = h / 168 + 1 iff start_k >= 1 and start_k <= w < start_k + weeks_k (start 0 = none);
 *          unit k is down iff word 2 + k < thr_k, thr_k = floor(for_rate_k * 2^32) clamped to [0, 2^32 - 1] (as relmc_hl1_load)
 *   hour:  in ascending unit order, skip units in maintenance or down; an ELU (finite limit) whose energy >= limit is exhausted and
 *          skipped, any other ELU adds its capacity to cap_elu; a non-ELU unit adds to cap_unl.  unserved = max(0, load - cap_unl).
 *          unserved > cap_elu: deficit = unserved - cap_elu, every available ELU's energy += its capacity;
 *          else unserved > 0: every available ELU's energy += unserved * (cap_i / cap_elu).
 *   year:  loss hours (deficit > 0), EUE (sum of deficits, hour order), loss events (rising edges of the loss flag, hour 0 counts).
 * Results depend only on (seed, year index, data), never on how a year range is split into calls; a repeated call is bitwise identical. */
#define RELMC_HL1_PLAN_MAX_ELU 8
/* Fleet (ngen <= 128 units, at most 8 of them with a finite energy_limit_mwh; INFINITY = not energy-limited), maintenance windows in
 * weeks (1-based start, 0 = none) and the hourly load curve of one year (1 <= nhours < 2^29), lfu_sigma_mw >= 0.  Held apart from the
 * relmc_hl1_load and relmc_hl1_seq_load models: none of the three calls disturbs the others. */
int32_t relmc_hl1_plan_load(relmc_ctx* ctx, int32_t ngen, const double* capacity_mw, const double* for_rate,
                            const int32_t* outage_start_week, const int32_t* outage_weeks, const double* energy_limit_mwh,
                            int32_t nhours, const double* hourly_load_mw, double lfu_sigma_mw);
/* years [first_year, first_year + n_years).  acc: sums over the years (lolf = loss events).  years_host: optional [n_years] (loss hours,
 * EUE, loss events).  hour_loss_count_host: optional [nhours], overwritten with this call's number of loss years per hour.
 * elu_energy_host: optional [n_years][n_elu], MWh used per ELU per year (ELUs in unit order). */
int32_t relmc_hl1_plan(relmc_ctx* ctx, uint64_t seed, uint64_t first_year, int64_t n_years, relmc_hl1_seq_acc* acc,
                       relmc_hl1_seq_year* years_host, int64_t* hour_loss_count_host, double* elu_energy_host);

/* ---- sequential HL2 (/root/reference/Montecarlo_seq/) ----------------- */
/* relmc_seq_load          <- seqmeantime() [MTTF MTTR] (seqmeantime.m:21-36) + the hourly load factors of
 *                            anloducurve (anloducurve.m:24-88, seqMain.m:67)
 * relmc_seq_mcsampling    <- seq_mcsampling(reliability_data, Ng, Nl, 1, hours) per year (seq_mcsampling.m:2;
 *                            every year starts all-up as seqMain.m:91): out[years][hours][ng+nl], 1 = down
 * relmc_seq_mcsimulation  <- [curt, nodal] = seq_mcsimulation(status, load_scale, ...) (seq_mcsimulation.m:1), batched
 * relmc_seq_run           <- the loop itself with its stopping rule and post-processing, seqMain.m:85-249 (below)
 * relmc_seq_years         <- the body of seqMain.m:85-176 for a range of simulated years, fused on the GPU:
 *                            chronology -> contingency hours (:97) -> DC-OPF per hour (:112-133) -> annual
 *                            indices (:160-176, calnlc.m) + the post-processing accumulators (:142-158)     */
typedef struct {
    double ens;               /* MWh, seqMain.m:173              */
    double dlc;               /* loss hours, :169                */
    double nlc;               /* loss events, :166 (calnlc)      */
    int64_t n_contingency;    /* hours evaluated, :103           */
} relmc_seq_year;
int32_t relmc_seq_load(relmc_ctx* ctx, const double* mttf, const double* mttr, int32_t hours_per_year,
                       const double* load_factors);
int32_t relmc_seq_mcsampling(relmc_ctx* ctx, uint64_t seed, uint64_t first_year, int32_t num_years,
                             uint8_t* state_host);
int32_t relmc_seq_mcsimulation(relmc_ctx* ctx, const uint8_t* states_host, const double* load_scale_host, int64_t n,
                               const relmc_solver_opts* opts, double* dns_host, double* nodal_host,
                               int32_t* status_host, int32_t* iters_host);
/* acc_out: n = LPs solved, n_fail = loss hours (curtailment > curtail_threshold, seqMain.m:41,144),
 * comp_fail = component-down counts during loss hours (:155), sum_nodal = nodal MWh over loss hours (:149) */
int32_t relmc_seq_years(relmc_ctx* ctx, uint64_t seed, uint64_t first_year, int32_t n_years,
                        const relmc_solver_opts* opts, double curtail_threshold, relmc_seq_year* years_out,
                        relmc_acc* acc_out);

/* ---- loss events of the sequential HL2 track: how often failures occur and how long they last (seqMain.m:15-16) ---- */
/* The years are relmc_seq_years' under the same arguments, word for word: same chronology, same hourly OPFs, same system curtailment
 * curt[h] per hour (0 on an hour without an outage and on an hour the pre-screen certifies).  System level only: the nodal split of a
 * curtailment is not a well-conditioned function of the data, so a per-bus threshold test has no defined answer.
 *   loss hour    an hour with curt[h] > curtail_threshold (strict, seqMain.m:140)
 *   loss event   a maximal run of consecutive loss hours inside one simulated year.  Years are independent and start all-up, and hour 0
 *                counts as a start (calnlc.m).  A run that reaches the year's last hour ends there and is flagged censored; it is an
 *                event like any other in every other field.
 * Per event: year relative to first_year, start_hour 0-based, duration in hours, energy_mwh = the sum of curt over its hours added left
 * to right in hour order, peak_mw the largest of them; onset = the components (bit k of word k / 32) that are down in the start hour and
 * were up in the hour before (in hour 0: every component that is down); involved = the OR of the down masks over the event's hours.
 * An event with an empty onset started without a new outage (a load rise) and is counted in load_onset_events.
 * So the events of a year number its nlc, their durations sum to its dlc, and their energies sum to at most its ens, with equality
 * iff no hour of the year has 0 < curt <= curtail_threshold. */
typedef struct {
    int32_t year;             /* relative to first_year */
    int32_t start_hour;       /* 0-based */
    int32_t duration;         /* hours */
    int32_t censored;         /* 1 if the run reaches the year's last hour */
    double energy_mwh, peak_mw;
    uint32_t onset[RELMC_MAX_COMP / 32];
    uint32_t involved[RELMC_MAX_COMP / 32];
} relmc_seq_event;
typedef struct {
    int64_t years, events, censored, load_onset_events, sum_dur, sum_dur2, max_dur;   /* years = simulated years; sums and maxima over the events */
    double sum_energy, sum_energy2, max_energy, max_peak;
    int64_t onset_events[RELMC_MAX_COMP];       /* events component k initiated (bit k of onset) */
    int64_t involved_events[RELMC_MAX_COMP];    /* events component k was down in (bit k of involved) */
    double onset_energy[RELMC_MAX_COMP];        /* MWh of the events it initiated, added in list order */
    double involved_energy[RELMC_MAX_COMP];     /* MWh of the events it was down in, added in list order */
} relmc_seq_event_acc;
/* years [first_year, first_year + n_years) of the chronology loaded by relmc_seq_load (RELMC_ERR_NO_CASE before that call).
 *   years_out, acc_out   as relmc_seq_years with the same arguments, byte for byte (one body serves both entries)
 *   ev_acc               required
 *   dur_hist_host        optional [n_dur_bins], 1 <= n_dur_bins <= 4096 when given (else RELMC_ERR_INVALID): dur_hist_host[d - 1] = events
 *                        with duration d for d < n_dur_bins, the last bin counts durations >= n_dur_bins; overwritten with this call's counts
 *   events_host          optional [events_cap], events_cap >= 0 (else RELMC_ERR_INVALID): the first min(ev_acc->events, events_cap) events
 *                        in (year, start_hour) order; ev_acc->events is always the true count, so a caller sees that its buffer was short
 * n_years == 0 zeroes the outputs.  Every output depends on (seed, year, options, data) only: a repeated call is bitwise identical;
 * splitting a year range into calls gives lists that concatenate (with `year` rebased), integer fields and histograms that add exactly
 * and maxima that combine by max; the floating-point sums are taken in a fixed order and agree to rounding across a split.
 * relmc_last_kernel_ms covers relmc_seq_years' kernels and the event kernels.  relmc_seq_run is unchanged and has no event output. */
int32_t relmc_seq_events(relmc_ctx* ctx, uint64_t seed, uint64_t first_year, int32_t n_years, const relmc_solver_opts* opts,
                         double curtail_threshold, relmc_seq_year* years_out, relmc_acc* acc_out, relmc_seq_event_acc* ev_acc,
                         int32_t n_dur_bins, int64_t* dur_hist_host, int64_t events_cap, relmc_seq_event* events_host);

/* relmc_seq_run <- the whole yearly loop of seqMain.m:85-199 (CoV stop at :194) and its post-processing :211-249, below the C ABI like
 * relmc_nsq_run.  With a communicator of more than one rank in the context (relmc_comm_init / relmc_comm_set_host_allreduce) it IS the
 * multi-rank loop: the years of every batch shard contiguously over the ranks, the annual triples are all-gathered in year order, every rank
 * stops at the same year and returns the same result.  The years depend on (seed, global year) only: results_year, the stopping year and every
 * integer of the accumulators do not depend on the number of ranks or on batch_years. */
typedef struct {
    double cov_threshold;     /* seqMain.m:40 (0.05) */
    int32_t max_years;        /* seqMain.m:39 (4000) */
    int32_t batch_years;      /* simulated years per launch round over all ranks; 0 = 64 per rank */
    uint64_t seed;
    double curtail_threshold; /* seqMain.m:41 (0.01 MW) */
    relmc_solver_opts solver;
    /* optional history buffers (may be NULL), each with room for years_cap >= max_years entries */
    int64_t years_cap;
    relmc_seq_year* results_year;   /* results_year.ens / dlc / nlc (+ contingency hours), seqMain.m:162-176 */
    double* cum_eens;               /* results_cum.eens, :180 */
    double* cum_cov;                /* results_cum.cov, :183-185 (entry 0 = 0 as in the reference; NaN = 0/0 while no year has had curtailment, as :184) */
} relmc_seq_opts;
typedef struct {
    int32_t final_year;       /* years simulated = the stopping year (seqMain.m:203) */
    int32_t converged;        /* CoV < cov_threshold reached (:194) */
    double eens;              /* MWh/yr, results_cum.eens(end)     */
    double cov;               /* results_cum.cov(end); NaN (0 / 0, as seqMain.m:184) if no simulated year had curtailment */
    double lole;              /* h/yr, mean(results_year.dlc), :212 */
    double lolf;              /* occ/yr, mean(results_year.nlc), :213 */
    double plc;               /* mean(results_year.plc)            */
    int64_t n_contingency;    /* contingency hours of the years 1..final_year (= hourly OPFs the run stands for) */
    relmc_acc acc;            /* accumulators over exactly the years 1..final_year: n = hourly OPFs, n_fail = loss hours (total_loss_hours, :158),
                                 comp_fail (:155), sum_nodal in MWh (:149) */
    double nodal_eens_avg[RELMC_MAX_BUS];      /* MWh/yr, :218 */
    double comp_importance[RELMC_MAX_COMP];    /* P(component down | loss hour), :233 */
    double wall_seconds, kernel_seconds;
} relmc_seq_result;
void relmc_seq_opts_default(relmc_seq_opts* opts);
int32_t relmc_seq_run(relmc_ctx* ctx, const relmc_seq_opts* opts, relmc_seq_result* result);

/* Units (samples, states, database rows) that the solver's static elimination order ends non-converged (status MAXIT or NUMFAIL;
 * 6.7e-7 of the RTS-96 scenarios, 4e-10 on RTS-24) are evaluated again under further static orders by every entry point, the
 * sequential ones included; the later attempt's results replace the first's.  Counters since relmc_case_load:
 * units re-evaluated, and how many of them ended converged (or MATPOWER-singular).  (The library reads ONE environment variable, RELMC_VERBOSE:
 * schedule statistics on stderr.  Diagnosis switches -- no second attempt, dense level first, one launch per batch -- exist as test hooks
 * only, relmc_debug_set in csrc/relmc_debug.hip.) */
int32_t relmc_retry_stats(const relmc_ctx* ctx, int64_t* units_out, int64_t* converged_out);
/* The kernel's list of non-converged units holds 4096 + (units of the call) / 256 entries (at most 2^20 to begin with).  relmc_nsq_accumulate / relmc_nsq_run
 * (every sample solved) evaluate a chunk again with a longer list if it overflows; the other entry points leave the units beyond the
 * list with their first-attempt results and count them here (0 on every case relmc_case_load calibrated: its primary order fails on at
 * most 0.1 % of the states). */
int32_t relmc_retry_overflow(const relmc_ctx* ctx, int64_t* units_out);
/* A unit that no static elimination order converges on is evaluated once more with every Newton step solved by Gaussian elimination
 * with PARTIAL PIVOTING on the dense reduced system (one scenario row per system, global scratch): what MATLAB's `\` does under MIPS
 * (mc_simulation.m:41).  Slow and rare (2 units in 1e9 RTS-96 samples reach it); its result takes the earlier attempts' place like theirs.
 * units_out / converged_out: how many units went there since the case was loaded and how many it converged on. */
int32_t relmc_retry_dense_stats(const relmc_ctx* ctx, int64_t* units_out, int64_t* converged_out);
/* relmc_case_load evaluates 8192 sampled states under the primary static order; a case on which more than 0.1 % of them end
 * non-converged gets the further orders probed on the same sample and the best of the three as its primary.  primary_out: 0 = the
 * default (level-then-fill), 1 = the same with the ties broken the other way, 2 = fill first; probe_failures_out: failures of each
 * probed order among the 8192 (-1 = not probed).  RTS-24 and RTS-96: {0, -1, -1}, nothing changes. */
int32_t relmc_case_order(const relmc_ctx* ctx, int32_t* primary_out, int32_t probe_failures_out[3]);
/* The primary order as a tunable of the schedule.  The Newton step of every scenario runs a static pass program that relmc_case_load
 * derives from the elimination order of the buses (MATLAB's `\` under mips picks its own pivot order per call, mc_simulation.m:41); the
 * built-in rule (shallow elimination tree first, then little fill) is good, an order searched against the scheduler itself is better:
 * RTS-24 174 -> 168 LDS instructions per Newton step (-1.4 % kernel time), RTS-96 215 -> 200 and 32 -> 28 dependent passes (-2.9 %).
 *   relmc_tune_order       host only (no device, no context): simulated annealing over bus permutations, `evaluations` runs of the scheduler
 *                          (3 ms each on RTS-96), deterministic in `seed`; start = NULL begins at the rule's order.  order_out[nb] = external
 *                          bus numbers in elimination order, the reference bus last; stats_out (optional) = {LDS instructions per Newton step,
 *                          dependent passes} of the start order and of the result.  An order never changes WHAT is computed, only the
 *                          rounding of the factorisation (iteration counts of single states may move by one).
 *                          The figures quoted above are those of the orders tuned for RTS-24 / RTS-96, which the hosts ship with their case data
 *                          (case24.RTS24_ELIM_ORDER / case96.RTS96_ELIM_ORDER, the same constants in julia/RelMC.jl); a host that passes no hint --
 *                          a plain C client -- runs the rule's order: same results to the solver's tolerances, another rounding.
 *   relmc_case_order_hint  the order for the NEXT relmc_case_load of this context (copied; NULL / 0 = the rule); the load fails with
 *                          RELMC_ERR_INVALID if it is not a permutation of 0..nb-1 with the reference bus last.  The further orders of
 *                          the retry path (relmc_retry_stats) stay rule-made. */
int32_t relmc_tune_order(const relmc_case_desc* desc, int32_t evaluations, uint64_t seed, const int32_t* start, int32_t* order_out, int32_t stats_out[4]);
int32_t relmc_case_order_hint(relmc_ctx* ctx, const int32_t* order, int32_t n);

/* ---- nsqMain (nsqMain.m:208-318 + 345-376) ------------------------------------------- */
/* Batches of up to 8192 samples (the reference's is 100, nsqMain.m:60) are evaluated many at a time in the modes
 * distinct_states = 0 and 2; every checkpoint's history entry and the stopping point are those of the batch-by-batch loop
 *  up to fp64 summation order: inside a stretch the checkpoints' EDNS / beta come from host sums of the per-sample dns
 * (the last checkpoint of a stretch, and with it the result, from the device accumulators themselves), which differ from the
 * batch-by-batch device sums in the last bits; integers (samples, loss counts, the stopping batch on any beta not within 1e-12 of its
 * limit) are identical.  A stretch that is cut at the stopping batch is evaluated again over the shorter range; its first evaluation
 * leaves no trace in relmc_retry_stats or kernel_seconds.  */
int32_t relmc_nsq_run(relmc_ctx* ctx, const relmc_nsq_opts* opts, relmc_nsq_result* result);

/* ---- importance sampling for the non-sequential HL2 Monte Carlo: cross-entropy tilt of the component unavailabilities (an extension beyond the reference) ---- */
/* nsqMain counts every sample with weight 1; away from the annual peak almost every sample is a zero.  Here the states are drawn under tilted
 * unavailabilities and every sample carries its likelihood ratio W, so that the weighted estimators stay unbiased for the case's own law.
 * Tilt.  unavail_is[ng+nl] = the sampling probabilities; NULL = the case's own.  thr_is[k] is derived from unavail_is[k] by exactly the rule
 *   relmc_case_load uses for thr[k] (relmc_case_thresholds): floor(u * 2^32), at most 2^32 - 1, and 0 where always_up.  A call is refused with
 *   RELMC_ERR_INVALID (relmc_last_error naming the component where the call takes a context) if an entry is not finite or outside [0, 1], or if
 *   thr_is[k] == 0 while thr[k] > 0: the tilted law must cover the nominal one.  A refused call changes nothing.
 * Draws.  relmc_mc_sampling's, word for word: Philox4x32-10, ctr = (index lo, index hi, k >> 2, 0), key = seed; component k is down iff word
 *   k & 3 < thr_is[k] (the spare words of the last block are ignored).  So with thr_is == thr the states are bitwise relmc_mc_sampling's, and
 *   with thr_is >= thr everywhere the down set of sample i contains the down set of the nominal sample i.
 * Weight.  From the realised probabilities thr / 2^32, not from the doubles that were passed in:
 *   r_dn[k] = (double)thr[k] / (double)thr_is[k]   (never read when thr_is[k] == 0: stored as 1.0)
 *   r_up[k] = (double)(2^32 - thr[k]) / (double)(2^32 - thr_is[k])
 *   each one fp64 division of exactly representable integers, done on the host.  W_i = the product over k ascending of r_dn[k] where component
 *   k of sample i is down and r_up[k] where it is up, starting from 1.0, one rounded multiply per component (no FMA): thr_is == thr gives
 *   W == 1.0 exactly, and a NumPy model reproduces every W bit for bit.  W is a plain fp64 product: an absurd tilt (hundreds of components at
 *   ratios far from 1) may underflow it to 0; relmc_nsq_is_tune's clamp [thr / 2^32, q_max] keeps it far from that.
 * Accumulators (relmc_is_acc), x_k = 1 iff component k is down, fail = dns > 1e-4 (nsqMain.m:270).  Every floating sum is taken in a fixed
 *   order: a repeated call is bitwise identical; splitting a range into calls changes the doubles only by rounding and the integers not at all. */
typedef struct {
    int64_t n;                /* samples evaluated                                   */
    int64_t n_fail;           /* raw count of dns > 1e-4                             */
    int64_t n_singular, n_infeasible, n_nonconverged, sum_iters;   /* as relmc_acc's */
    double sum_w, sum_w2;     /* sum W, sum W^2                                      */
    double sum_wfail, sum_w2fail;   /* sum W fail, sum W^2 fail                      */
    double sum_wdns, sum_w2dns2;    /* sum W dns, sum (W dns)^2                      */
    double comp_wfail[RELMC_MAX_COMP];   /* sum W fail x_k                           */
    double comp_wdns[RELMC_MAX_COMP];    /* sum W dns x_k                            */
    double sum_wnodal[RELMC_MAX_BUS];    /* sum W nodal_dns                          */
} relmc_is_acc;
/* relmc_nsq_indices' formulas with W dns in place of dns and W fail in place of fail; with every W = 1 each field the two structs share equals
 * relmc_nsq_indices' output. */
typedef struct {
    int64_t n;
    double edns;              /* sum_wdns / n                                        */
    double lole;              /* plc * hours_per_year                                */
    double plc;               /* sum_wfail / n                                       */
    double beta;              /* relmc_nsq_indices' expression fed sum_wdns, sum_w2dns2 */
    double eens;              /* edns * hours_per_year                               */
    double mean_iters;
    double beta_plc;          /* the same expression fed sum_wfail, sum_w2fail       */
    double mean_w;            /* sum_w / n: 1 in expectation                         */
    double ess;               /* effective sample size sum_w^2 / sum_w2              */
    double nodal_eens[RELMC_MAX_BUS];        /* sum_wnodal / n                       */
    double comp_importance[RELMC_MAX_COMP];  /* comp_wfail / sum_wfail, 0 without a failure */
} relmc_is_indices;
/* Host only (no context, no GPU): the validation above and the three tables [ncomp].  thr = relmc_case_thresholds' output; always_up and
 * unavail_is may be NULL (nothing forced / the nominal law: thr_is = thr).  Returns RELMC_ERR_INVALID for a refused tilt;
 * bad_component_out (optional) = the offending component, -1 if none. */
int32_t relmc_is_ratios(int32_t ncomp, const uint32_t* thr, const uint8_t* always_up, const double* unavail_is,
                        uint32_t* thr_is_out, double* r_dn_out, double* r_up_out, int32_t* bad_component_out);
/* States eqstatus[n x (ng+nl)] (row-major, 1 = failed) and weights W[n] of samples [first_index, first_index + n); either output may be NULL. */
int32_t relmc_is_sampling(relmc_ctx* ctx, uint64_t seed, uint64_t first_index, int64_t n, const double* unavail_is,
                          uint8_t* eqstatus_host, double* weight_host);
int32_t relmc_is_sampling_dev(relmc_ctx* ctx, uint64_t seed, uint64_t first_index, int64_t n, const double* unavail_is,
                              uint8_t* eqstatus_dev, double* weight_dev);
/* Samples the range under the tilt, evaluates the states through relmc_mc_simulation_dev (retry ladder included) and reduces, in launches of
 * at most 2^20 samples so that the per-sample buffers stay bounded.  relmc_last_kernel_ms covers sampling, every evaluation launch and the
 * reductions.  opts->screen is ignored: relmc_mc_simulation solves every state it is handed (certifying tilted samples is a follow-up).
 * n == 0 zeroes *out; RELMC_ERR_NO_CASE before relmc_case_load. */
int32_t relmc_nsq_is_accumulate(relmc_ctx* ctx, uint64_t seed, uint64_t first_index, int64_t n, const relmc_solver_opts* opts,
                                const double* unavail_is, relmc_is_acc* out);
void relmc_is_acc_zero(relmc_is_acc* acc);
void relmc_is_acc_merge(relmc_is_acc* dst, const relmc_is_acc* src);
void relmc_nsq_is_indices(const relmc_is_acc* acc, int32_t nb, int32_t ncomp, double hours_per_year, relmc_is_indices* out);
/* The cross-entropy tuner.  Pass t = 0, 1, ... samples the indices [t * n_pilot, (t + 1) * n_pilot) of `seed` under the current tilt q (pass 0:
 * the nominal p_k = thr[k] / 2^32) and evaluates them.  F = its samples with dns > 1e-4.
 *   |F| >= min_elite (a FINAL pass): elites = F with weight e_i = W_i (objective 0, PLC) or W_i dns_i (objective 1, EDNS).
 *   otherwise (a LEVEL pass): elites = F plus the ceil(rho * n_pilot) - |F| non-failed samples of largest generation shortfall
 *     m_i = total_load - sum over the in-service real generators, ascending, of max(inj_pmax, 0)   (ties: the lower index), e_i = W_i.
 *   update: v_k = sum_i e_i x_ik / sum_i e_i (sum_i e_i on the host in sample order, the column sums on the device, by the kernel that produces
 *     comp_wfail / comp_wdns);  q_k <- min(alpha v_k + (1 - alpha) q_k, q_max), then max(., p_k), and 0 where always_up: never below nominal.
 *     A pass without an elite of positive weight leaves q as it is.
 * Stops after final_iters final passes or max_iters passes; never reaching a final pass is reported (report->final_passes == 0), not an error.
 * Deterministic in (seed, options, case): a repeated call is bitwise identical.  unavail_is_out[ng+nl] = the tilt, report optional. */
#define RELMC_IS_TUNE_MAX_PASSES 32
typedef struct {
    uint64_t seed;
    int64_t n_pilot;          /* 20000 */
    int32_t max_iters;        /* 5, at most RELMC_IS_TUNE_MAX_PASSES */
    int32_t final_iters;      /* 2 */
    int64_t min_elite;        /* 100 */
    double rho;               /* 0.1, in (0, 1] */
    int32_t objective;        /* 0 = PLC, 1 = EDNS */
    int32_t reserved;         /* 0 */
    double alpha;             /* smoothing, 1.0, in (0, 1] */
    double q_max;             /* 0.5, in (0, 1] */
    relmc_solver_opts solver;
} relmc_is_tune_opts;
typedef struct {
    int32_t passes;           /* passes run */
    int32_t final_passes;     /* how many of them were final */
    int64_t n_fail[RELMC_IS_TUNE_MAX_PASSES];      /* |F| per pass */
    int64_t n_elite[RELMC_IS_TUNE_MAX_PASSES];     /* elites per pass */
    double sum_e[RELMC_IS_TUNE_MAX_PASSES];        /* sum of e_i per pass */
    double level[RELMC_IS_TUNE_MAX_PASSES];        /* level pass: the smallest shortfall among the added elites (MW); NaN for a final pass or none added */
    double kernel_seconds, wall_seconds;
} relmc_is_tune_report;
void relmc_is_tune_opts_default(relmc_is_tune_opts* opts);
int32_t relmc_nsq_is_tune(relmc_ctx* ctx, const relmc_is_tune_opts* opts, double* unavail_is_out, relmc_is_tune_report* report);
/* Batches of `batch` samples of `seed` from index 0 under unavail_is until beta <= beta_limit or max_samples; histories optional, one entry
 * per batch, as in relmc_nsq_run.  Single-rank: RELMC_ERR_UNSUPPORTED with a communicator of more than one rank in the context. */
typedef struct {
    double beta_limit;        /* 0.0017 */
    int64_t max_samples;      /* 1e5    */
    int64_t batch;            /* 1000   */
    uint64_t seed;
    double hours_per_year;    /* 8760   */
    relmc_solver_opts solver;
    const double* unavail_is; /* [ng+nl] or NULL = nominal */
    int64_t history_cap;
    double* beta_history;
    double* edns_history;
    double* plc_history;
} relmc_is_run_opts;
typedef struct {
    relmc_is_acc acc;
    relmc_is_indices idx;
    int64_t checkpoints;      /* history entries written = min(batches, history_cap) */
    int64_t batches;
    int32_t converged;        /* beta <= beta_limit */
    int32_t reserved;
    double wall_seconds, kernel_seconds;
} relmc_is_run_result;
void relmc_is_run_opts_default(relmc_is_run_opts* opts);
int32_t relmc_nsq_is_run(relmc_ctx* ctx, const relmc_is_run_opts* opts, relmc_is_run_result* result);

#ifdef __cplusplus
}
#endif
#endif /* RELMC_H */
