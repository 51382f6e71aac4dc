// relmc_nsq_run.hip — the nsqMain loop itself (relmc_nsq_run, nsqMain.m:208-318) for any number of ranks, in two forms: checkpoint stretches for
// small batches, one evaluation per batch otherwise; and the rule that says how long a stretch is (stretch_length).  Host code only.
#include <chrono>
#include <cmath>
#include <cstring>

#include "relmc_ctx.h"

namespace relmc_host {

// How long a stretch?  beta falls like 1 / sqrt(n), so the run will need about done * (beta / limit)^2 samples: go to 90 % of that in
// one stretch, then to 103 % of the (then better) prediction -- a stretch that is cut is taken again over its used part, so the last one
// should be short (round 3: beta < 1 % at the reference's batch of 100 in 5.9 instead of 9.4 ms; doubling stretches evaluated 416 k
// samples for a run of 211 k).  Without a prediction (first stretch, no loss yet, limit 0): ~25 600 samples, then as many as the run holds.
// Never more than `per` samples (the buffer of per-sample dns), never fewer than ~1600 with a prediction; always whole batches.
// round > 0 (the fused form: samples of one round of the grid):  a launch costs as many rounds as its busiest wavefront walks scenario groups:
// 24 576 samples are three groups for every wavefront of the 16-lane tile's grid, 25 600 make some walk a fourth (0.45 against 0.60 ms).
// Stretches that are not the last one end just below a whole number of rounds (in whole batches); the last one keeps its length -- it has
// to reach the stopping point.
Stretch stretch_length(int64_t batch, int64_t done, double beta, double beta_limit, int64_t per, int64_t round)
{
    const int64_t first = 25600 / batch > 0 ? 25600 / batch * batch : batch;      // ~25 600 samples, whole batches
    const int64_t least = 1600 / batch > 0 ? 1600 / batch * batch : batch;
    Stretch s = {done > first ? done / batch * batch : first, false};
    if (done > 0 && beta_limit > 0.0 && beta < 1e6 && beta > beta_limit) {
        const double need = (double)done * (beta / beta_limit) * (beta / beta_limit);
        s.final = !((double)done < 0.85 * need);
        const double target = s.final ? 1.03 * need : 0.9 * need;
        const double l = std::ceil((target - (double)done) / (double)batch) * (double)batch;
        s.len = l < (double)least ? least : (l > (double)per ? per : (int64_t)l);
    }
    if (s.len > per) s.len = per;
    if (round > 0 && !s.final) {
        const int64_t snapped = (s.len / round) * round / batch * batch;
        if (s.len >= 2 * round && snapped >= least) s.len = snapped;
    }
    return s;
}

}  // namespace relmc_host

using namespace relmc_host;

extern "C" {

// nsqMain.m:208-318: batches until beta <= beta_limit or max_samples, then the post-processing of :345-376.
// More than one rank (relmc_comm_init / relmc_comm_set_host_allreduce): every range [lo0, lo0 + len) of the global sample stream is split
// contiguously over the ranks, each evaluates its slice, ONE all-reduce per range (the convergence check), and every rank computes the same
// indices and stops at the same batch -- the parfor of nsqMain.m:257-263 with the loop around it, so that a C, Julia or MATLAB host calls
// this one function on every rank.  One rank is the case in which the slice is the whole range and no collective is entered.  The sampler is
// keyed by (seed, global index): the integers of the result do not depend on the number of ranks, the fp64 sums only in their summation order.
int32_t relmc_nsq_run(relmc_ctx* ctx, const relmc_nsq_opts* o, relmc_nsq_result* res)
{
    if (!ctx) return RELMC_ERR_INVALID;
    if (!ctx->has_case) return fail(ctx, RELMC_ERR_NO_CASE, "relmc_nsq_run: no case loaded");
    if (!o || !res || o->batch <= 0 || o->max_samples <= 0) return fail(ctx, RELMC_ERR_INVALID, "relmc_nsq_run: bad options");
    std::memset(res, 0, sizeof(*res));
    const auto t0 = std::chrono::steady_clock::now();
    const int nb = ctx->nb, ncomp = ctx->ncomp;
    const int64_t R = comm_ranks(ctx), r = R > 1 ? ctx->comm_rank : 0;
    const bool use_db = o->distinct_states == 2;
    double beta = INFINITY, kernel_ms = 0.0;
    int64_t done = 0, cp = 0;
    if (use_db) { const int rc0 = relmc_db_reset(ctx); if (rc0) return rc0; }
    auto checkpoint = [&](const relmc_indices& ix) {
        if (cp < o->history_cap) {
            if (o->beta_history) o->beta_history[cp] = ix.beta;
            if (o->edns_history) o->edns_history[cp] = ix.edns;
            if (o->lole_history) o->lole_history[cp] = ix.lole;
            if (o->plc_history) o->plc_history[cp] = ix.plc;
        }
        cp++;
    };
    // Small batches (the reference's own is 100 samples, nsqMain.m:60) would make every checkpoint one launch of a nearly empty grid and one
    // collective.  They are evaluated a STRETCH of whole batches at a time instead: every rank evaluates its slice of the stretch with the dns
    // of each of its samples and folds it into per-checkpoint (sum dns, sum dns^2, losses) triples -- all that the four indices of a checkpoint
    // need (nsqMain.m:286-301); ONE all-reduce of 3 x checkpoints + the accumulators (as doubles: the counts are exact below 2^53) gives every
    // rank every checkpoint; all ranks walk the same checkpoints and cut at the same one.  A cut stretch is taken again over its used part
    // (the database first put back to its rows and counts of before the stretch; one more all-reduce), so that the result is the one of the
    // batch-by-batch loop.  Only for batches whose launch is overhead-bound (a launch costs 0.2-0.4 ms whatever its size, i.e. as much as 1e4
    // scenarios), with stretches sized from the run's own beta on every rank alike: what a cut throws away stays a few per cent of the run.
    // The state database is per rank and keeps the per-batch loop over several ranks (a cut would have to rewind every rank's).
    if (o->batch <= kStretchMaxBatch && !ctx->sw.nsq_no_stretch /* diagnosis: one launch per batch */ &&
        (o->distinct_states == 0 || (use_db && R == 1))) {
        const int64_t per = stretch_per(o->batch);                // buffer size = longest stretch
        const int64_t round = use_db ? 0 : (int64_t)ctx->num_cu * ctx->blocks_per_cu * (ctx->tile == 0 ? Tile24::WPB * Tile24::SPW : Tile96::WPB * Tile96::SPW);
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        HIP_TRY(ctx, ctx->hist.d.grow((size_t)per));
        HIP_TRY(ctx, ctx->hist.h.grow((size_t)per));
        constexpr int64_t NI = (int64_t)(offsetof(relmc_acc, sum_dns) / sizeof(int64_t)), ND = (int64_t)((sizeof(relmc_acc) - offsetof(relmc_acc, sum_dns)) / sizeof(double));
        const double* const hd = ctx->hist.h.get();
        std::vector<double> box;                                  // [3 x checkpoints | with several ranks: the accumulators, integers first]
        // this rank's samples [lo, lo + cnt): the fused pass, or the database trio; accumulators into *part (the database's are taken from its
        // rows at the end of the stretch), with dns the dns of every sample in ctx->hist.h
        auto evaluate = [&](int64_t lo, int64_t cnt, bool dns, relmc_acc* part) -> int {
            int rc = use_db && dns ? db_snapshot(ctx) : RELMC_OK;
            if (rc) return rc;
            rc = use_db ? relmc_nsq_db_batch(ctx, o->seed, (uint64_t)lo, cnt, &o->solver, nullptr, nullptr)
                        : nsq_accumulate_impl(ctx, o->seed, (uint64_t)lo, cnt, &o->solver, part, dns ? ctx->hist.d.get() : nullptr);
            if (rc) return rc;
            kernel_ms += ctx->last_kernel_ms;
            if (!dns) return RELMC_OK;
            rc = use_db ? db_sample_dns(ctx, o->seed, (uint64_t)lo, cnt, ctx->hist.d.get()) : RELMC_OK;
            if (rc) return rc;
            if (hipMemcpyAsync(ctx->hist.h.get(), ctx->hist.d.get(), sizeof(double) * (size_t)cnt, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
                hipStreamSynchronize(ctx->stream) != hipSuccess) return fail(ctx, RELMC_ERR_HIP, "relmc_nsq_run: copy of the per-sample dns failed");
            return RELMC_OK;
        };
        // [lo0, lo0 + len) over the ranks: *out = its accumulators and, with ncp > 0, box[0, 3 ncp) = the triples of its ncp checkpoints
        auto shared_eval = [&](int64_t lo0, int64_t len, int64_t ncp, relmc_acc* out) -> int {
            const int64_t lo = lo0 + len * r / R, cnt = lo0 + len * (r + 1) / R - lo, off = lo - lo0;
            relmc_acc_zero(out);
            const int rc = cnt > 0 ? evaluate(lo, cnt, ncp > 0, out) : RELMC_OK;
            box.assign((size_t)(3 * ncp + (R > 1 ? NI + ND : 0)), 0.0);
            // a checkpoint's sums start at 0 and take its samples in sampling order (one that two ranks share gets two partial sums)
            if (rc == RELMC_OK && ncp > 0) for (int64_t i = 0; i < cnt;) {
                const int64_t k = (off + i) / o->batch, end = (k + 1) * o->batch - off < cnt ? (k + 1) * o->batch - off : cnt;
                double sd = 0.0, sd2 = 0.0; int64_t nf = 0;
                for (; i < end; ++i) { const double v = hd[(size_t)i]; sd += v; sd2 = std::fma(v, v, sd2); nf += v > 1e-4 /* nsqMain.m:270 */; }
                box[(size_t)(3 * k)] = sd; box[(size_t)(3 * k + 1)] = sd2; box[(size_t)(3 * k + 2)] = (double)nf;
            }
            if (R == 1) return rc;
            double* const q = &box[(size_t)(3 * ncp)];
            int64_t* const ai = reinterpret_cast<int64_t*>(out); double* const ad = &out->sum_dns;
            const std::string local_err = ctx->err;
            if (rc == RELMC_OK) {
                for (int64_t k = 0; k < NI; ++k) q[k] = (double)ai[k];
                for (int64_t k = 0; k < ND; ++k) q[NI + k] = ad[k];
            } else q[0] = NAN;                                    // a rank whose slice failed still enters the collective and says so where every rank looks
            const int rc_ar = comm_allreduce_f64(ctx, box.data(), (int64_t)box.size());
            if (rc != RELMC_OK) { ctx->err = local_err; return rc; }
            if (rc_ar) return rc_ar;
            if (q[0] != q[0]) return fail(ctx, RELMC_ERR_HIP, "relmc_nsq_run: another rank failed to evaluate its slice of the stretch (see that rank's relmc_last_error)");
            for (int64_t k = 0; k < NI; ++k) ai[k] = (int64_t)std::llround(q[k]);
            for (int64_t k = 0; k < ND; ++k) ad[k] = q[NI + k];
            return RELMC_OK;
        };
        while (beta > o->beta_limit && done < o->max_samples) {
            const int64_t len = stretch_length(o->batch, done, beta, o->beta_limit, per, round).len;
            const int64_t m = (o->max_samples - done) < len ? (o->max_samples - done) : len;
            const int64_t ncp = (m + o->batch - 1) / o->batch;
            const int64_t rows0 = ctx->db.n, samples0 = ctx->db.samples;
            // what a stretch that is cut and taken again must not count twice: its second attempts, its kernel time
            const RetryMark mark(ctx);
            const double kernel_ms0 = kernel_ms;
            relmc_acc part;
            int rc = shared_eval(done, m, ncp, &part);
            if (rc) return rc;
            relmc_acc run = res->acc;                       // only n, n_fail, sum_dns, sum_dns2 are advanced per checkpoint
            int64_t used = 0;
            for (int64_t k = 0; k < ncp; ++k) {
                const int64_t b = (m - used) < o->batch ? (m - used) : o->batch;
                const double* t = &box[(size_t)(3 * k)];
                if (R == 1 && t[0] != t[0]) return fail(ctx, RELMC_ERR_HIP, "relmc_nsq_run: a sampled state is missing from the database");
                run.n += b; run.n_fail += (int64_t)std::llround(t[2]); run.sum_dns += t[0]; run.sum_dns2 += t[1];
                used += b;
                relmc_indices ix;
                relmc_nsq_indices(&run, 0, 0, o->hours_per_year, &ix);
                beta = ix.beta;
                checkpoint(ix);
                if (beta <= o->beta_limit) break;
            }
            if (used < m) {            // cut, on every rank (they all see the same beta): the discarded stretch leaves no trace in the bookkeeping ...
                mark.restore(ctx);
                kernel_ms = kernel_ms0;
                rc = use_db ? db_rewind(ctx, rows0, samples0) : RELMC_OK;       // ... nor in the database; then the shorter range
                if (rc == RELMC_OK) rc = shared_eval(done, used, 0, &part);
                if (rc) return rc;
            }
            if (use_db) {
                const auto t1 = std::chrono::steady_clock::now();
                rc = db_accumulate(ctx, &res->acc);                    // nsqMain.m:282-301 over all rows
                if (rc) return rc;
                kernel_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
            } else relmc_acc_merge(&res->acc, &part);
            done += used;
            // the stretch's last checkpoint from the accumulators themselves (what the caller is handed), not from the host sums
            relmc_nsq_indices(&res->acc, nb, ncomp, o->hours_per_year, &res->idx);
            beta = res->idx.beta;
            cp--;
            checkpoint(res->idx);
        }
    }
    else
    // One evaluation and one all-reduce of the accumulators per batch.  The state database (the reference's own loop body: persistent
    // unique-state database, indices recomputed from all of its rows) is per rank -- each rank's rows are the states of ITS slices --, and its
    // accumulators are cumulative, so they are all-reduced and taken as they are.
    while (beta > o->beta_limit && done < o->max_samples) {
        const int64_t m = (o->max_samples - done) < o->batch ? (o->max_samples - done) : o->batch;
        const int64_t lo = done + m * r / R, cnt = done + m * (r + 1) / R - lo;
        relmc_acc part;
        relmc_acc_zero(&part);
        int rc = RELMC_OK;
        if (use_db) rc = relmc_nsq_db_batch(ctx, o->seed, (uint64_t)lo, cnt, &o->solver, &part, nullptr);
        else if (cnt > 0) rc = o->distinct_states ? relmc_nsq_accumulate_distinct(ctx, o->seed, (uint64_t)lo, cnt, &o->solver, &part, nullptr)
                                                  : relmc_nsq_accumulate(ctx, o->seed, (uint64_t)lo, cnt, &o->solver, &part);
        if (rc == RELMC_OK && (cnt > 0 || use_db)) kernel_ms += ctx->last_kernel_ms;
        if (R > 1) {
            // a rank whose slice failed still enters the collective (the others would wait for it for ever) and says so in a counter no
            // evaluation ever makes negative: every rank then returns an error from the same batch
            const std::string local_err = ctx->err;
            if (rc != RELMC_OK) { relmc_acc_zero(&part); part.n_nonconverged = -((int64_t)1 << 40); }
            const int rc_ar = relmc_comm_allreduce_acc(ctx, &part);
            if (rc != RELMC_OK) { ctx->err = local_err; return rc; }
            if (rc_ar) return rc_ar;
            if (part.n_nonconverged < 0) return fail(ctx, RELMC_ERR_HIP, "relmc_nsq_run: another rank failed to evaluate its slice of the batch (see that rank's relmc_last_error)");
        } else if (rc) return rc;
        if (use_db) res->acc = part; else relmc_acc_merge(&res->acc, &part);
        done += m;
        relmc_nsq_indices(&res->acc, nb, ncomp, o->hours_per_year, &res->idx);
        beta = res->idx.beta;
        checkpoint(res->idx);
    }
    res->checkpoints = cp < o->history_cap ? cp : o->history_cap;     // history entries written
    res->batches = cp;
    res->converged = beta <= o->beta_limit ? 1 : 0;
    res->kernel_seconds = kernel_ms * 1e-3;
    res->wall_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    ctx->last_kernel_ms = kernel_ms;
    return RELMC_OK;
}

}  // extern "C"
